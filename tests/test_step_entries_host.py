"""What every `ops` step wrapper hands to the library, argument by argument: the C entry's name and its full positional tuple
against literals, for the twelve scheduler-step wrappers and the two window wrappers, at a size the eight-element kernels take
(inner = 24, per = 96) and one they do not (inner = 15, per = 60).  A recording object stands in for the library: CPU only."""
import ctypes

import pytest
import torch

f16, f32 = torch.float16, torch.float32
SIZES = {"vec8": (2, 4, 3, 2, 4), "scalar": (2, 4, 3, 1, 5)}
G, S = 7.5, 0.875                                       # guidance scale, next_input_scale
K = (1.5, 0.25, 0.75, 0.125, 0.5)                       # k_x, k_eps, c_x0, c_xt, sigma / c_prev: all exact in fp32
LEVEL = (0.625, 0.375)                                  # a_next, s_next
STARTS, PROFILE = [0, 1], [1.0, 3.0]                    # two windows of two frames over the three frames


class RecordingLib:
    def __init__(self):
        self.recorded = []

    def __getattr__(self, name):
        return lambda *args: self.recorded.append((name, args)) or 0


@pytest.fixture
def lib(monkeypatch):
    from lavie_amd import _lib, ops
    rec = RecordingLib()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "check", lambda rc, *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    monkeypatch.setattr(ops, "_chk16", lambda *ts: None)       # the tensors here live on the CPU
    monkeypatch.setattr(ops, "_chk32", lambda *ts: None)
    return rec


def operands(shape):
    p, c, f = shape[:3]
    win = (c, 2) + shape[3:]
    t = dict(x=torch.zeros(shape, dtype=f32), noise=torch.zeros(shape, dtype=f32), x0_prev=torch.zeros(shape, dtype=f32),
             known=torch.zeros(shape, dtype=f32), noise_known=torch.zeros(shape, dtype=f32),
             mask=torch.zeros((p, 1) + shape[2:], dtype=f32), table=torch.zeros(p, 2, dtype=f32),
             wtable=torch.zeros(2, p, 2, dtype=f32))
    for name, nb in (("eps", p), ("model_in", p), ("eps2", 2 * p), ("model_in2", 2 * p)):
        t[name] = torch.zeros((nb,) + shape[1:], dtype=f16)
        for w in range(2):
            t[f"{name}_w{w}"] = torch.zeros((nb,) + win, dtype=f16)
    return t


def pointer_names(t):
    return {v.data_ptr(): k for k, v in t.items()}


def described(value, names):
    """One recorded argument as something a literal can state: a pointer as the name of the tensor it points at, a struct passed by
    reference as the dict of its fields, numbers as they are."""
    if isinstance(value, ctypes.c_void_p):
        return names[value.value]
    if hasattr(value, "_obj"):                              # ctypes.byref(struct)
        s, out = value._obj, {}
        for field, ftype in s._fields_:
            v = getattr(s, field)
            if ftype is ctypes.c_void_p:                    # read back as an int, or None when null
                v = names[v] if v else None
            if field in ("starts_host", "profile_host"):
                n = s.W if field == "starts_host" else s.L
                v = [v[i] for i in range(n)]
            elif field in ("eps_host", "model_in_host"):
                v = [names[v[i]] for i in range(s.W)]
            elif isinstance(v, ctypes._Pointer) or isinstance(v, ctypes.c_void_p):
                addr = ctypes.cast(v, ctypes.c_void_p).value
                v = names[addr] if addr else None
            out[field] = v
        return out
    return value


def region(shape, noise_known="noise_known"):
    inner = shape[2] * shape[3] * shape[4]
    return dict(struct_size=48, channels=4, inner=inner, known="known", mask="mask", noise_known=noise_known, a_next=0.625, s_next=0.375)


def window_args(shape, family, cfg, aux, guidance):
    eps, mi = ("eps2", "model_in2") if cfg else ("eps", "model_in")
    return dict(struct_size=120, family=family, cfg=cfg, P=2, C=4, F=3, hw=shape[3] * shape[4], W=2, L=2, starts_host=[0, 1],
                profile_host=[1.0, 3.0], eps_host=[f"{eps}_w0", f"{eps}_w1"], model_in_host=[f"{mi}_w0", f"{mi}_w1"], x="x", aux=aux,
                guidance=guidance, k_x=1.5, k_eps=0.25, c_x0=0.75, c_xt=0.125, c4=0.5, next_input_scale=0.875)


KN = ("known", "mask", "noise_known", LEVEL)            # what a wrapper around known latents takes after next_input_scale
# wrapper -> (its arguments, tensors by name; the entry; the positional tuple as a function of (n, per, shape))
CASES = {
    "cfg_ddpm_step": (("eps2", "x", "noise", "model_in2", G, K, S), "lavie_cfg_sampler_step",
                      lambda n, per, sh: ("eps2", "x", "noise", "model_in2", n, 7.5, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream")),
    "sampler_step": (("eps", "x", "noise", "model_in", K, S), "lavie_sampler_step",
                     lambda n, per, sh: ("eps", "x", "noise", "model_in", n, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream")),
    "cfg_multistep_step": (("eps2", "x", "x0_prev", "model_in2", G, K, S), "lavie_cfg_multistep_step",
                           lambda n, per, sh: ("eps2", "x", "x0_prev", "model_in2", n, 7.5, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream")),
    "multistep_step": (("eps", "x", "x0_prev", "model_in", K, S), "lavie_multistep_step",
                       lambda n, per, sh: ("eps", "x", "x0_prev", "model_in", n, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream")),
    "cfg_sampler_step_known": (("eps2", "x", "noise", "model_in2", G, K, S) + KN, "lavie_cfg_sampler_step_known",
                               lambda n, per, sh: ("eps2", "x", "noise", "model_in2", n, 7.5, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream",
                                                   region(sh))),
    "sampler_step_known": (("eps", "x", "noise", "model_in", K, S) + KN, "lavie_sampler_step_known",
                           lambda n, per, sh: ("eps", "x", "noise", "model_in", n, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream", region(sh))),
    "cfg_multistep_step_known": (("eps2", "x", "x0_prev", "model_in2", G, K, S) + KN, "lavie_cfg_multistep_step_known",
                                 lambda n, per, sh: ("eps2", "x", "x0_prev", "model_in2", n, 7.5, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875,
                                                     "stream", region(sh))),
    "multistep_step_known": (("eps", "x", "x0_prev", "model_in", K, S) + KN, "lavie_multistep_step_known",
                             lambda n, per, sh: ("eps", "x", "x0_prev", "model_in", n, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875, "stream",
                                                 region(sh))),
    "cfg_sampler_step_scaled": (("eps2", "x", "noise", "model_in2", "table", K, S), "lavie_cfg_sampler_step_scaled",
                                lambda n, per, sh: ("eps2", "x", "noise", "model_in2", n, "table", per, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875,
                                                    "stream")),
    "cfg_multistep_step_scaled": (("eps2", "x", "x0_prev", "model_in2", "table", K, S), "lavie_cfg_multistep_step_scaled",
                                  lambda n, per, sh: ("eps2", "x", "x0_prev", "model_in2", n, "table", per, 1.5, 0.25, 0.75, 0.125, 0.5, 0.875,
                                                      "stream")),
    "cfg_sampler_step_known_scaled": (("eps2", "x", "noise", "model_in2", "table", K, S) + KN, "lavie_cfg_sampler_step_known_scaled",
                                      lambda n, per, sh: ("eps2", "x", "noise", "model_in2", n, "table", 1.5, 0.25, 0.75, 0.125, 0.5, 0.875,
                                                          "stream", region(sh))),
    "cfg_multistep_step_known_scaled": (("eps2", "x", "x0_prev", "model_in2", "table", K, S) + KN, "lavie_cfg_multistep_step_known_scaled",
                                        lambda n, per, sh: ("eps2", "x", "x0_prev", "model_in2", n, "table", 1.5, 0.25, 0.75, 0.125, 0.5,
                                                            0.875, "stream", region(sh))),
}


def call(ops, wrapper, args, t, **kw):
    getattr(ops, wrapper)(*[t[a] if isinstance(a, str) else a for a in args], **kw)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("wrapper", list(CASES))
def test_step_wrapper_passes_these_arguments(lib, wrapper, size):
    from lavie_amd import ops
    shape = SIZES[size]
    t = operands(shape)
    args, entry, want = CASES[wrapper]
    call(ops, wrapper, args, t)
    (name, got), = lib.recorded
    n = t["x"].numel()
    assert n == {"vec8": 192, "scalar": 120}[size]
    assert name == entry
    assert tuple(described(v, pointer_names(t)) for v in got) == want(n, n // 2, shape)


@pytest.mark.parametrize("size", list(SIZES))
def test_optional_operands_travel_as_null(lib, size):
    """sigma == 0 runs pass no noise; a region whose landing level has no noise part passes no noise_known"""
    from lavie_amd import ops
    shape = SIZES[size]
    t = operands(shape)
    n = t["x"].numel()
    ops.cfg_ddpm_step(t["eps2"], t["x"], None, t["model_in2"], G, K[:4] + (0.0,))
    ops.sampler_step_known(t["eps"], t["x"], None, t["model_in"], K[:4] + (0.0,), 1.0, t["known"], t["mask"], None, (1.0, 0.0))
    ops.cfg_sampler_step_scaled(t["eps2"], t["x"], None, t["model_in2"], t["table"], K[:4] + (0.0,))
    got = [(name, tuple(described(v, pointer_names(t)) for v in a)) for name, a in lib.recorded]
    r = dict(region(shape, None), a_next=1.0, s_next=0.0)
    assert got == [("lavie_cfg_sampler_step", ("eps2", "x", None, "model_in2", n, 7.5, 1.5, 0.25, 0.75, 0.125, 0.0, 1.0, "stream")),
                   ("lavie_sampler_step_known", ("eps", "x", None, "model_in", n, 1.5, 0.25, 0.75, 0.125, 0.0, 1.0, "stream", r)),
                   ("lavie_cfg_sampler_step_scaled", ("eps2", "x", None, "model_in2", n, "table", n // 2, 1.5, 0.25, 0.75, 0.125, 0.0, 1.0,
                                                      "stream"))]


WINDOW_CASES = {
    "guided": (dict(guidance=G, multistep=False), "noise", lambda sh: window_args(sh, 0, 1, "noise", 7.5)),
    "unguided": (dict(guidance=None, multistep=False), "noise", lambda sh: window_args(sh, 0, 0, "noise", 1.0)),
    "guided-multistep": (dict(guidance=G, multistep=True), "x0_prev", lambda sh: window_args(sh, 1, 1, "x0_prev", 7.5)),
    "no-noise": (dict(guidance=G, multistep=False), None, lambda sh: window_args(sh, 0, 1, None, 7.5)),
}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", list(WINDOW_CASES))
def test_window_step_passes_these_arguments(lib, case, size):
    from lavie_amd import ops
    shape = SIZES[size]
    t = operands(shape)
    kw, aux, want = WINDOW_CASES[case]
    half = "2" if kw["guidance"] is not None else ""
    eps, mi = [t[f"eps{half}_w{w}"] for w in range(2)], [t[f"model_in{half}_w{w}"] for w in range(2)]
    ops.window_step(eps, t["x"], t[aux] if aux else None, mi, STARTS, PROFILE, kw["guidance"], K, S, multistep=kw["multistep"])
    (name, got), = lib.recorded
    assert name == "lavie_window_step"
    assert tuple(described(v, pointer_names(t)) for v in got) == (want(shape), "stream")


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("multistep", [False, True])
def test_window_step_scaled_passes_these_arguments(lib, multistep, size):
    from lavie_amd import ops
    shape = SIZES[size]
    t = operands(shape)
    aux = "x0_prev" if multistep else "noise"
    eps, mi = [t[f"eps2_w{w}"] for w in range(2)], [t[f"model_in2_w{w}"] for w in range(2)]
    ops.window_step_scaled(eps, t["x"], t[aux], mi, STARTS, PROFILE, t["wtable"], K, S, multistep=multistep)
    (name, got), = lib.recorded
    assert name == "lavie_window_step_scaled"
    assert tuple(described(v, pointer_names(t)) for v in got) == (window_args(shape, int(multistep), 1, aux, 1.0), "wtable", "stream")
