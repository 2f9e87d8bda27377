"""Seeded engine noise, the host side (no GPU): the library's Philox4x32-10 against the numpy restatement and Random123's
known-answer vectors, the sample moments of the float64 reference, `PhiloxGenerator`, `StepNoise` / `step` / `window_step` with
it (a recording object stands in for `ops`), and the refusals of the C entries with pointers that are never dereferenced."""
import ctypes

import numpy as np
import pytest
import torch

import noise_reference as R
from lavie_amd import _lib, ops, sampling
from lavie_amd.noise import NoiseKey, PhiloxGenerator


# ------------------------------------------------------------------ 1. the integer stream
def test_known_answer_vectors():
    for counter, key, want in R.KAT:
        assert tuple(int(v) for v in R.philox4x32_10(key, counter)) == want
        assert tuple(ops.philox4x32(key, counter)) == want


def test_library_equals_restatement_on_random_inputs():
    rng = np.random.default_rng(20240607)
    keys = rng.integers(0, 2 ** 32, size=(1000, 2), dtype=np.uint64)
    counters = rng.integers(0, 2 ** 32, size=(1000, 4), dtype=np.uint64)
    want = R.philox4x32_10(keys, counters)
    for k, c, w in zip(keys.tolist(), counters.tolist(), want.tolist()):
        assert ops.philox4x32(k, c) == w


def test_philox_host_refuses_null():
    lib = _lib.load()
    assert lib.lavie_philox4x32_host(None, None, None) != 0 and b"null" in lib.lavie_last_error()


# ------------------------------------------------------------------ 2. moments of the float64 reference
MOMENT_SEED = 1234


def test_reference_moments():
    """5 sigma bounds of the sample moments of N(0, 1) at N = 2^20: var(mean) = 1 / N, var(m2) = 2 / N, var(m4) = 96 / N."""
    n = 1 << 20
    z = R.normal(MOMENT_SEED, 0, 0, n)
    mean, var, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    print(f"mean={mean:.3e} var-1={var - 1:.3e} m4-3={m4 - 3:.3e}")
    assert np.isfinite(z).all()
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)


def test_reference_addressing():
    """a slice equals that range of the whole, also across the low counter word; draws and seeds differ"""
    whole = R.normal(7, 3, 0, 64)
    assert np.array_equal(R.normal(7, 3, 5, 11), whole[5:16])
    first = 2 ** 34 - 3
    assert np.array_equal(R.normal(7, 3, first, 8)[2:], R.normal(7, 3, first + 2, 6))
    assert not np.array_equal(R.normal(7, 4, 0, 64), whole) and not np.array_equal(R.normal(8, 3, 0, 64), whole)


# ------------------------------------------------------------------ 3. PhiloxGenerator
def test_seed_expansion():
    assert PhiloxGenerator(10).seeds(3) == [10, 11, 12] == PhiloxGenerator([10, 11, 12]).seeds(3)
    assert PhiloxGenerator(-1).seeds(2) == [2 ** 64 - 1, 0]               # seeds are 64-bit words
    assert PhiloxGenerator(2 ** 64 - 1).seeds(2) == [2 ** 64 - 1, 0]
    with pytest.raises(ValueError, match="2 seeds for 3 latents"):
        PhiloxGenerator([1, 2]).seeds(3)
    with pytest.raises(ValueError, match="empty"):
        PhiloxGenerator([])
    for bad in (1.5, "7", None, True):
        with pytest.raises(TypeError):
            PhiloxGenerator(bad)


def test_counter_advances_by_one_per_draw_for_all_latents():
    g = PhiloxGenerator(5)
    assert g.key(4) == NoiseKey([5, 6, 7, 8], 0)
    assert g.key(4) == NoiseKey([5, 6, 7, 8], 1)
    assert g.next_draw() == 2 and g.draw == 3


def test_split_and_slices_share_the_counter():
    g = PhiloxGenerator(100)
    g.next_draw()
    a, b = g.split([2, 3])
    assert a.seeds(2) == [100, 101] and b.seeds(3) == [102, 103, 104] and a.draw == b.draw == 1
    assert g[1:2].seeds(1) == [101] and g[3:].seeds(2) == [103, 104]
    a.next_draw()
    assert (a.draw, b.draw, g.draw) == (2, 1, 1)                          # each part counts on its own afterwards
    h = PhiloxGenerator([9, 4, 7])
    x, y = h.split([1, 2])
    assert x.seeds(1) == [9] and y.seeds(2) == [4, 7] and h[1:3].seeds(2) == [4, 7]
    assert h[1:2].seeds(1) == [4] == PhiloxGenerator(4).seeds(1)          # prompt b of a batch = the single call with its seed
    with pytest.raises(ValueError, match="covers 2 latents"):
        h.split([1, 1])
    with pytest.raises(ValueError):
        h.split([3, 0])
    with pytest.raises(TypeError):
        h[0]
    with pytest.raises(TypeError):
        h[::2]


class RecordingOps:
    """Stands in for `lavie_amd.ops` inside `sampling`: records (name, args)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args, **kw):
            self.calls.append((name, args, kw))
            return kw.get("out")
        return record


@pytest.fixture
def rec(monkeypatch):
    r = RecordingOps()
    monkeypatch.setattr(sampling, "ops", r)
    return r


def test_step_noise_with_a_philox_generator_allocates_no_tensors(rec, monkeypatch):
    x = torch.zeros(3, 4, 2, 2, 2)
    made = []
    for name in ("empty", "empty_like", "zeros", "randn"):
        monkeypatch.setattr(torch, name, lambda *a, _n=name, **k: made.append(_n) or (_ for _ in ()).throw(AssertionError(_n)))
    noise = sampling.StepNoise(x, PhiloxGenerator(40))
    d0, d1 = noise.draw(), noise.draw()
    noise.done()
    assert made == [] and rec.calls == []
    assert not hasattr(noise, "_noise") and not hasattr(noise, "_pinned") and not hasattr(noise, "_side")
    assert d0.key == NoiseKey([40, 41, 42], 0) and d1.key == NoiseKey([40, 41, 42], 1)


def test_step_noise_refuses_a_seed_list_of_another_length():
    with pytest.raises(ValueError, match="2 seeds for 3 latents"):
        sampling.StepNoise(torch.zeros(3, 4, 2, 2, 2), PhiloxGenerator([1, 2]))


def test_step_passes_the_key_where_a_fused_form_exists_and_the_tensor_elsewhere(rec):
    x = torch.zeros(2, 4, 2, 2, 2)
    noise = sampling.StepNoise(x, PhiloxGenerator([11, 12]))
    K = (1.0, 0.5, 0.3, 0.7, 0.1)
    sampling.step("eps", x, noise.draw(), "min", None, K, 1.0, False)
    sampling.step("eps", x, noise.draw(), "min", 7.5, K, 1.0, False)
    assert [(c[0], c[1][2]) for c in rec.calls] == [("sampler_step_seeded", NoiseKey([11, 12], 0)),
                                                    ("cfg_sampler_step_seeded", NoiseKey([11, 12], 1))]
    assert rec.calls[1][1] == ("eps", x, NoiseKey([11, 12], 1), "min", 7.5, K, 1.0)
    rec.calls.clear()
    # a known region, PAG: the tensor, from ops.philox_normal into ONE buffer
    region = ("known", "mask", "kn", (1.0, 0.0))
    sampling.step("eps", x, noise.draw(), "min", 7.5, K, 1.0, False, region)
    sampling.step("eps", x, noise.draw(), "min", sampling.PagGuidance(7.5, 3.0), K, 1.0, False)
    names = [c[0] for c in rec.calls]
    assert names == ["philox_normal", "cfg_sampler_step_known", "philox_normal", "cfg_pag_sampler_step"]
    assert rec.calls[0][1] == ([11, 12], 32, 2) and rec.calls[2][1] == ([11, 12], 32, 3)
    buf = rec.calls[0][2]["out"]
    assert buf is rec.calls[2][2]["out"] and tuple(buf.shape) == tuple(x.shape) and buf.dtype == torch.float32
    assert rec.calls[1][1][2] is buf and rec.calls[3][1][2] is buf


def test_window_step_passes_the_key(rec):
    x = torch.zeros(2, 4, 5, 2, 2)
    noise = sampling.StepNoise(x, PhiloxGenerator(3))
    K = (1.0, 0.5, 0.3, 0.7, 0.1)
    sampling.window_step(["e0", "e1"], x, noise.draw(), ["m0", "m1"], [0, 2], [1.0, 2.0, 1.0], 7.5, K, 0.9, False)
    (name, args, kw), = rec.calls
    assert name == "window_step_seeded" and args == (["e0", "e1"], x, NoiseKey([3, 4], 0), ["m0", "m1"], [0, 2], [1.0, 2.0, 1.0], 7.5, K, 0.9)


def test_randn_tensor_draws_through_ops(monkeypatch):
    from lavie_amd import scheduling_ddpm
    seen = []

    def philox_normal(seeds, per, draw, first_element=0, out=None, device="cuda"):
        seen.append((seeds, per, draw, str(device)))
        return torch.zeros(len(seeds), per)
    monkeypatch.setattr(ops, "philox_normal", philox_normal)
    g = PhiloxGenerator(8)
    t = scheduling_ddpm.randn_tensor((2, 4, 3, 2, 2), generator=g, device="cpu")
    scheduling_ddpm.randn_tensor((2, 3, 3, 4, 4), generator=g, device="cpu")
    assert tuple(t.shape) == (2, 4, 3, 2, 2) and seen == [([8, 9], 48, 0, "cpu"), ([8, 9], 144, 1, "cpu")]


def test_from_sample_yaml_noise_key():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"seed": 77}, unet=object())
    assert "generator" not in kw                                          # torch stays the default
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"seed": 77, "noise": "torch"}, unet=object())
    assert "generator" not in kw
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"seed": 77, "noise": "engine"}, unet=object())
    assert isinstance(kw["generator"], PhiloxGenerator) and kw["generator"].seeds(2) == [77, 78]
    with pytest.raises(ValueError, match="noise"):
        VideoGenPipeline.from_sample_yaml({"noise": "curand"}, unet=object())


# ------------------------------------------------------------------ the C entries' refusals, before any device call
BASE = 1 << 20             # fake device addresses: never dereferenced, every refusal comes before a HIP call


def make_key(count=2, per=24, draw=0, seeds=(1, 2), **over):
    k = _lib.NoiseKeyC()
    k.struct_size = ctypes.sizeof(_lib.NoiseKeyC)
    arr = (ctypes.c_ulonglong * max(len(seeds), 1))(*seeds)
    k.count, k.seeds_host, k.per, k.draw = count, arr, per, draw
    for name, v in over.items():
        setattr(k, name, v)
    return k, arr


def test_seeded_entries_refuse_by_name():
    lib = _lib.load()
    ok = [ctypes.c_void_p(BASE * i) for i in (1, 2, 3)]
    good = (1.0, 0.5, 0.3, 0.7, 0.1, 0.9)

    def refused(word, rc):
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    def cfg(key, n=48, ptrs=ok, scalars=good):
        return lib.lavie_cfg_sampler_step_seeded(*ptrs, n, 7.5, *scalars, None, key)

    def one(key, n=48, ptrs=ok, scalars=good):
        return lib.lavie_sampler_step_seeded(*ptrs, n, *scalars, None, key)

    for call in (cfg, one):
        refused("key is null", call(None))
        k, keep = make_key(struct_size=8)
        refused("struct_size", call(ctypes.byref(k)))
        for count in (0, 17, -1):
            k, keep = make_key(count=count)
            refused(f"key->count={count}", call(ctypes.byref(k)))
        k, keep = make_key()
        k.seeds_host = None
        refused("seeds_host is null", call(ctypes.byref(k)))
        k, keep = make_key(per=0)
        refused("key->per=0", call(ctypes.byref(k)))
        k, keep = make_key()
        refused("n=47 is not key->count=2 latents", call(ctypes.byref(k), n=47))
        for i, name in enumerate(("eps", "x", "model_in")):
            ptrs = list(ok)
            ptrs[i] = None
            refused(f"{name} is null", call(ctypes.byref(k), ptrs=ptrs))
    # the materialised form
    seeds = (ctypes.c_ulonglong * 17)(*range(17))
    f = lib.lavie_philox_normal_f32
    refused("out is null", f(None, seeds, 2, 8, 0, 0, None))
    refused("seeds_host is null", f(ok[0], None, 2, 8, 0, 0, None))
    refused("P=0", f(ok[0], seeds, 0, 8, 0, 0, None))
    refused("P=17", f(ok[0], seeds, 17, 8, 0, 0, None))
    refused("per=0", f(ok[0], seeds, 2, 0, 0, 0, None))
    refused("first_element=-1", f(ok[0], seeds, 2, 8, -1, 0, None))
    refused("first_element=", f(ok[0], seeds, 2, 8, (1 << 62) - 7, 0, None))
    refused("4-byte", f(ctypes.c_void_p(BASE + 2), seeds, 2, 8, 0, 0, None))
    assert lib.lavie_abi_version() == 8                                   # additive: the ABI version did not move


def test_launchers_refuse_a_key_beside_an_operand_without_a_seeded_form():
    """launch_step / launch_window_step themselves, through the test hook: no C entry can hand them these combinations.  Each refusal
    names what the key was combined with; nothing is launched (the process has no device)."""
    lib = _lib.load()
    want = {1: "sampler step: a noise key is not combined with `known` (a known region)",
            2: "sampler step: a noise key is not combined with `table` (a guidance table)",
            3: "sampler step: a noise key is not combined with `eps_pag` (perturbed-attention guidance)",
            4: "seeded sampler step: the multistep family draws no noise and takes no noise key",
            5: "window step: a noise key is not combined with `table` (a guidance table)",
            6: "window step: the multistep family draws no noise and takes no noise key"}
    for combine, text in want.items():
        rc = lib.lavie_debug_noise_key_refusal(combine)
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and msg.startswith(text), (combine, rc, msg)
    for combine in (0, 7, -1):
        assert lib.lavie_debug_noise_key_refusal(combine) != 0 and f"combine={combine}" in lib.lavie_last_error().decode()


def test_window_step_seeded_refuses_by_name():
    from test_windows_host import C, F, HW, P, make_args
    lib = _lib.load()

    def refused(word, a, k):
        rc = lib.lavie_window_step_seeded(ctypes.byref(a) if a is not None else None, ctypes.byref(k) if k is not None else None, None)
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and word in msg, (word, rc, msg)

    a, keep = make_args()
    k, arr = make_key(count=P, per=C * F * HW, seeds=(5,))
    refused("key is null", a, None)
    refused("args is null", None, k)
    bad, arr2 = make_key(count=P, per=C * F * HW + 1, seeds=(5,))
    refused("key->count=1 per=209", a, bad)
    bad, arr2 = make_key(count=2, per=C * F * HW, seeds=(5, 6))
    refused("the clip has P=1", a, bad)
    m, keep2 = make_args(family=1)
    refused("multistep family draws no noise", m, k)
    n, keep3 = make_args(aux=None)                                        # aux is not needed: refused for another reason
    n.x = None
    refused("x is null", n, k)


def test_ops_seeded_wrappers_refuse_by_name():
    x = torch.zeros(2, 4, 2, 2, 2)
    h = torch.zeros(2, 4, 2, 2, 2, dtype=torch.float16)
    with pytest.raises(ValueError, match="fp16 device"):
        ops.sampler_step_seeded(h, x, NoiseKey([1, 2], 0), h, (1, 1, 1, 0, 0))
    with pytest.raises(ValueError, match="must be >= 1"):
        ops.philox_normal([], 8, 0)
