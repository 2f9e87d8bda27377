"""Guidance from a per-latent table on the GPU (csrc/sampler_guidance.hip and the table forms of sampler_known.hip /
sampler_window.hip): per element against the float64 model of guidance_reference.py on guarded, poisoned operands (opcheck.py), the
bit guarantees, and the pipelines with `guidance_rescale` / per-prompt `guidance_scale` against test-side fp32 oracle loops that apply
rescale_noise_cfg written from its published formula.  Parity with diffusers' own function is not pinned: the package is not
available to the tests.  Every test here needs the new entry points or keywords and fails without them."""
import pytest
import torch

import guidance_cases as C
import guidance_reference as R
import opcheck as oc

pytestmark = pytest.mark.gpu

f16, f32t = torch.float16, torch.float32
FORMS = ("plain", "known")
FAMILIES = ("five", "multistep")


@pytest.fixture(scope="module")
def ops():
    from lavie_amd import ops as o
    return o


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. chunk sums and the table
def table_of(ops, eps, p, guidance, phi):
    """(table [P, 2], moments [P, 4]) on the CPU, from un-guarded operands."""
    mom = torch.empty(p, 4, dtype=torch.float64, device="cuda")
    tab = ops.guidance_table(eps.cuda(), p, guidance, phi, moments_out=mom)
    return tab.cpu(), mom.cpu()


@pytest.mark.parametrize("name,offset", [(n, 0.0) for n in C.SHAPES] + [("2x3CH", 2.0)])
def test_chunk_sums_and_table_vs_float64(ops, name, offset):
    p, per = C.SHAPES[name][0], C.per_of(name)
    d = C.inputs(name, offset)
    g = list(C.GUIDANCE[:p])
    chunks = R.launch_rule(p, per)["chunks"]
    assert ops.guidance_partials_floats(p, per) == p * chunks * 4
    mom = torch.empty(p, 4, dtype=torch.float64, device="cuda")
    g_dev = torch.tensor(g, dtype=f32t, device="cuda")

    def run(i, o):
        ops.guidance_table(i["eps"], p, g_dev, C.PHI, workspace=o["partials"], out=o["table"], moments_out=mom)

    res = oc.run_guarded(run, {"eps": d["eps"]}, {"partials": ((p * chunks * 4,), f32t), "table": ((p, 2), f32t)}, sync=sync)
    eu, ec = d["eps"][:p].reshape(p, per), d["eps"][p:].reshape(p, per)
    worst = R.check_chunk_sums(res["partials"].reshape(p, chunks, 4), eu, ec, g, label=name)
    sums = mom.cpu()
    R.check_latent_sums(sums, eu, ec, g, label=name)
    rel = R.check_table(res["table"], sums, per, g, C.PHI, label=name)      # the table from the double sums read back
    print(f"{name} offset {offset}: chunk sums worst |err| / bound {worst:.3f}; f = {res['table'][:, 1].tolist()}, worst |f - f64| / |f64| {rel:.3e}")
    # and f itself against the published formula on the fp32 predictions (the unbiased torch.std), loosely: the sums are fp32
    e = R.guided_e32(eu, ec, g).double()
    want = C.PHI * ec.double().std(1) / e.std(1) + (1 - C.PHI)
    if per >= 64:
        assert bool(((res["table"][:, 1].double() - want).abs() <= 1e-4 * want).all())


def test_degenerate_statistics(ops):
    """All-zero predictions: s_e == 0 gives f = 1 (diffusers gives NaN).  rescale = 0: f = 1, the partials are not touched."""
    eps = torch.zeros(4, 4, 105, dtype=f16, device="cuda")
    tab = ops.guidance_table(eps, 2, [5.0, 9.0], 0.7)
    assert tab.cpu().tolist() == [[5.0, 1.0], [9.0, 1.0]]
    ws = torch.full((ops.guidance_partials_floats(2, 420),), 7.0, device="cuda")
    tab = ops.guidance_table(torch.randn(4, 4, 105, device="cuda").half(), 2, 7.5, 0.0, workspace=ws)
    assert tab.cpu().tolist() == [[7.5, 1.0], [7.5, 1.0]] and bool((ws == 7.0).all())


# ------------------------------------------------------------------ 2. the four steps on [P, C, inner]
def step_call(ops, form, family, i, o, table, guidance=None):
    """The scaled step (table given) or the plain step of the same family and form (guidance given)."""
    name = ("cfg_multistep_step" if family == "multistep" else "cfg_sampler_step") + ("_known" if form == "known" else "")
    if table is None and name == "cfg_sampler_step":
        name = "cfg_ddpm_step"
    region = (i["known"], i["mask"], i["noise_known"], C.LEVEL) if form == "known" else ()
    fn = getattr(ops, name + ("_scaled" if table is not None else ""))
    fn(i["eps"], i["x"], i["aux"], o["model_in"], table if table is not None else guidance, C.COEFFS[family], C.IN_SCALE, *region)


def step_operands(d, form, p):
    ins = {k: d[k] for k in ("eps", "x", "aux") + (("known", "mask", "noise_known") if form == "known" else ())}
    outs = {"model_in": (tuple(d["eps"].shape), f16), "x": (tuple(d["x"].shape), f32t), "aux": (tuple(d["x"].shape), f32t)}
    return ins, outs


def run_step(ops, name, form, family, table_cpu=None, guidance=None, d=None):
    p = C.SHAPES[name][0]
    d = d or C.inputs(name)
    ins, outs = step_operands(d, form, p)
    alias = {"x": "x", "aux": "aux"}
    if family == "five":
        outs.pop("aux")
        alias.pop("aux")
    if table_cpu is not None:
        ins["table"] = table_cpu

    def run(i, o):
        step_call(ops, form, family, i, o, i.get("table"), guidance)

    return oc.run_guarded(run, ins, outs, alias=alias, sync=sync)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_scaled_step_per_element_vs_float64(ops, name, form, family):
    """x, the history and every element of both halves of model_in, with the table read back."""
    p, c, inner = C.SHAPES[name]
    per = c * inner
    d = C.inputs(name)
    table, _ = table_of(ops, d["eps"], p, list(C.GUIDANCE[:p]), C.PHI)
    res = run_step(ops, name, form, family, table_cpu=table)
    eps, m_eps = R.scaled_eps64(d["eps"][:p].reshape(p, per), d["eps"][p:].reshape(p, per), table)
    shape = d["x"].shape
    xn, m, x0, m0 = R.step64(family, eps.reshape(shape), m_eps.reshape(shape), d["x"], d["aux"], C.COEFFS[family])
    kinds = (family, "history")
    if form == "known":
        xn, m, x0, m0 = R.known64(family, xn, m, x0, m0, d["known"], d["mask"].expand(shape), d["noise_known"], C.LEVEL)
        kinds = ("known_" + family, "known_history")
    oc.assert_elementwise(res["x"], xn, m, 2 * R.ROUNDINGS[kinds[0]] * R.U32, label=f"{name} {form} {family} x", u=0.0)
    if family == "multistep":
        oc.assert_elementwise(res["aux"], x0, m0, 2 * R.ROUNDINGS[kinds[1]] * R.U32, label=f"{name} {form} {family} x0_prev", u=0.0)
    oc.assert_bits(res["model_in"].reshape(2, -1), R.model_input(family, res["x"].reshape(1, -1), C.IN_SCALE), label="model_in")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["3x420", "2x(CH+8)", "1x8"])
def test_table_of_g_and_one_is_the_plain_kernel_bit_for_bit(ops, name, form, family):
    """(g, 1.0) in every row: the bits of the plain kernel of the family in x, the history and model_in, both routes."""
    p = C.SHAPES[name][0]
    table = torch.tensor([[7.5, 1.0]] * p, dtype=f32t)
    got = run_step(ops, name, form, family, table_cpu=table)
    want = run_step(ops, name, form, family, guidance=7.5)
    for k in want:
        oc.assert_bits(got[k], want[k], label=f"{name} {form} {family} {k}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
def test_a_latent_of_a_batch_equals_its_own_call(ops, form, family):
    """P = 3 with scales (g0, g1, g2) and phi = 0.7: latent p has the bits of the P = 1 call on that latent with the scalar g_p and the
    same phi, table entry included.  Run twice: identical."""
    name = "3x420"
    p = 3
    d = C.inputs(name)
    g = list(C.GUIDANCE)

    def whole(dd, gs, n):
        dev = {k: v.cuda() for k, v in dd.items()}
        dev["aux"], out = dev["aux"].clone(), {"model_in": torch.empty_like(dev["eps"])}
        table = ops.guidance_table(dev["eps"], n, gs, C.PHI)
        step_call(ops, form, family, dev, out, table)
        return table.cpu(), dev["x"].cpu(), dev["aux"].cpu(), out["model_in"].cpu()

    batch, again = whole(d, g, p), whole(d, g, p)
    for a, b in zip(batch, again):
        assert torch.equal(a, b)
    for q in range(p):
        one = {k: (torch.cat([v[q:q + 1], v[p + q:p + q + 1]]) if k == "eps" else v[q:q + 1]).contiguous() for k, v in d.items()}
        table, x, aux, mi = whole(one, g[q], 1)
        assert torch.equal(table[0], batch[0][q]) and torch.equal(x[0], batch[1][q]) and torch.equal(aux[0], batch[2][q])
        assert torch.equal(mi[0], batch[3][q]) and torch.equal(mi[1], batch[3][p + q]) and torch.equal(mi[0], mi[1])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
def test_a_nan_poisoned_latent_poisons_exactly_its_own_outputs(ops, form, family):
    """One NaN among latent 1's prompt predictions: its table entry is NaN, and x, the multistep history and both halves of model_in
    are NaN in latent 1 wherever the prediction reaches them (everywhere in the plain form; around known latents everywhere but
    the elements the mask pins, which keep the clean run's bits).  Latents 0 and 2 keep the clean run's bits, table included."""
    name = "3x420"
    p = 3
    d = dict(C.inputs(name))
    eps = d["eps"].clone()
    eps[p + 1, 2, 17] = float("nan")
    outs = []
    for e in (d["eps"], eps):
        dev = {k: v.cuda() for k, v in d.items()}
        dev["eps"] = e.cuda()
        o = {"model_in": torch.empty_like(dev["eps"])}
        table = ops.guidance_table(dev["eps"], p, list(C.GUIDANCE), C.PHI)
        step_call(ops, form, family, dev, o, table)
        outs.append((table.cpu(), dev["x"].cpu(), dev["aux"].cpu(), o["model_in"].cpu()))
    (t0, x0, a0, m0), (t1, x1, a1, m1) = outs
    assert bool(t1[1, 1].isnan()) and torch.equal(t1[[0, 2]], t0[[0, 2]]) and float(t1[1, 0]) == C.GUIDANCE[1]
    reached = torch.ones_like(x0[1], dtype=torch.bool) if form == "plain" else (d["mask"][1] != 1.0).expand_as(x0[1])
    assert bool(reached.any()) and (form == "plain" or bool((~reached).any()))
    tensors = [(x0, x1)] + ([(a0, a1)] if family == "multistep" else []) + [(m0[:p], m1[:p]), (m0[p:], m1[p:])]
    for clean, dirty in tensors:
        assert torch.equal(dirty[[0, 2]], clean[[0, 2]])
        assert bool(dirty[1][reached].isnan().all()) and torch.equal(dirty[1][~reached], clean[1][~reached])
    if family == "five":
        assert torch.equal(a1, a0)                    # the step's noise is only read


# ------------------------------------------------------------------ 3. the windowed step
def window_run(ops, hw, family, table_cpu=None, guidance=None):
    w = C.WINDOWS
    d = C.window_inputs(hw)
    from lavie_amd.windows import window_profile
    profile = window_profile(w["L"], "triangle")
    n_win = len(w["starts"])
    ins = {"x": d["x"], "aux": d["aux"], **{f"eps{k}": e for k, e in enumerate(d["eps"])}}
    outs = {"x": (tuple(d["x"].shape), f32t), **{f"model_in{k}": (tuple(d["eps"][0].shape), f16) for k in range(n_win)}}
    alias = {"x": "x"}
    if family == "multistep":
        outs["aux"], alias["aux"] = (tuple(d["x"].shape), f32t), "aux"
    if table_cpu is not None:
        ins["table"] = table_cpu

    def run(i, o):
        eps, mi = [i[f"eps{k}"] for k in range(n_win)], [o[f"model_in{k}"] for k in range(n_win)]
        if table_cpu is not None:
            ops.window_step_scaled(eps, i["x"], i["aux"], mi, w["starts"], profile, i["table"], C.COEFFS[family], C.IN_SCALE,
                                   multistep=family == "multistep")
        else:
            ops.window_step(eps, i["x"], i["aux"], mi, w["starts"], profile, guidance, C.COEFFS[family], C.IN_SCALE,
                            multistep=family == "multistep")

    return oc.run_guarded(run, ins, outs, alias=alias, sync=sync), d, profile


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("hw", C.WINDOWS["hws"])
def test_window_step_with_a_table(ops, hw, family):
    """P 2, C 4, F 6, L 4, starts [0, 2]: one guidance_table call over both windows, then the scaled step, per element; a table of
    (g, 1) gives the plain windowed kernel's bits."""
    import window_reference as W
    w = C.WINDOWS
    d = C.window_inputs(hw)
    table = ops.guidance_table([e.cuda() for e in d["eps"]], w["P"], list(C.GUIDANCE[:2]), C.PHI).cpu()
    assert table.shape == (2, 2, 2) and not torch.equal(table[0, :, 1], table[1, :, 1])      # a factor of its own per window
    for k, e in enumerate(d["eps"]):                                                         # = the single-window tables
        assert torch.equal(table[k], table_of(ops, e, w["P"], list(C.GUIDANCE[:2]), C.PHI)[0])
    res, _, profile = window_run(ops, hw, family, table_cpu=table)
    xn, m, x0, m0 = R.window64(family, d["eps"], d["x"], d["aux"], w["starts"], profile, table, C.COEFFS[family])
    k = W.bound_k(family if family == "multistep" else "five", w["F"], w["L"], w["starts"]) + 2.0
    oc.assert_elementwise(res["x"], xn, m * k.expand(xn.shape), R.U32, label=f"window {hw} {family} x", u=0.0)
    if family == "multistep":
        kh = W.bound_k("history", w["F"], w["L"], w["starts"]) + 2.0
        oc.assert_elementwise(res["aux"], x0, m0 * kh.expand(xn.shape), R.U32, label=f"window {hw} {family} x0_prev", u=0.0)
    for j, s in enumerate(w["starts"]):
        want = R.model_input(family, res["x"][:, :, s:s + w["L"]].reshape(1, -1), C.IN_SCALE)
        oc.assert_bits(res[f"model_in{j}"].reshape(2, -1), want, label=f"model_in[{j}]")
    ones = torch.tensor([[[7.5, 1.0]] * w["P"]] * 2, dtype=f32t)
    got, want = window_run(ops, hw, family, table_cpu=ones)[0], window_run(ops, hw, family, guidance=7.5)[0]
    for name in want:
        oc.assert_bits(got[name], want[name], label=f"window {hw} {family} {name}")


@pytest.mark.parametrize("family", FAMILIES)
def test_a_nan_in_one_window_poisons_its_latent_in_the_frames_that_window_covers(ops, family):
    """A NaN in window 1's prompt prediction of latent 0: table[1, 0] is NaN and no other entry; latent 0 is NaN in frames 2..5
    (window 1) in x, the history and both windows' model inputs there; frames 0, 1 and all of latent 1 keep the clean run's bits."""
    from lavie_amd.windows import window_profile
    w, hw = C.WINDOWS, 8
    d = C.window_inputs(hw)
    profile = window_profile(w["L"], "triangle")
    bad = [d["eps"][0], d["eps"][1].clone()]
    bad[1][w["P"] + 0, 1, 2, 3] = float("nan")
    outs = []
    for eps in (d["eps"], bad):
        eps = [e.cuda() for e in eps]
        x, aux, mi = d["x"].cuda(), d["aux"].cuda(), [torch.empty_like(e) for e in eps]
        table = ops.guidance_table(eps, w["P"], list(C.GUIDANCE[:2]), C.PHI)
        ops.window_step_scaled(eps, x, aux, mi, w["starts"], profile, table, C.COEFFS[family], C.IN_SCALE, multistep=family == "multistep")
        outs.append((table.cpu(), x.cpu(), aux.cpu(), [m.cpu() for m in mi]))
    (t0, x0, a0, m0), (t1, x1, a1, m1) = outs
    nan = t1.isnan()
    assert nan.nonzero().tolist() == [[1, 0, 1]] and torch.equal(t1[~nan], t0[~nan])
    lo = w["starts"][1]
    clips = [(x0, x1)] + ([(a0, a1)] if family == "multistep" else [])
    for clean, dirty in clips:
        assert bool(dirty[0, :, lo:].isnan().all()) and torch.equal(dirty[0, :, :lo], clean[0, :, :lo]) and torch.equal(dirty[1], clean[1])
    for k, s in enumerate(w["starts"]):
        for half in (0, w["P"]):
            got, want = m1[k][half:half + w["P"]], m0[k][half:half + w["P"]]
            hit = torch.tensor([s + f >= lo for f in range(w["L"])])
            assert bool(got[0][:, hit].isnan().all()) and torch.equal(got[0][:, ~hit], want[0][:, ~hit]) and torch.equal(got[1], want[1])


def test_wrapper_refusals(ops):
    eps, x = torch.zeros(2, 4, 8, dtype=f16, device="cuda"), torch.zeros(1, 4, 8, device="cuda")
    mi, table = torch.empty_like(eps), torch.ones(1, 2, device="cuda")
    with pytest.raises(ValueError, match="rescale"):
        ops.guidance_table(eps, 1, 7.5, 1.5)
    with pytest.raises(ValueError, match="guidance scales"):
        ops.guidance_table(eps, 1, [7.5, 3.0], 0.5)
    with pytest.raises(ValueError, match="workspace"):
        ops.guidance_table(eps, 1, 7.5, 0.5, workspace=torch.empty(3, device="cuda"))
    with pytest.raises(ValueError, match="table"):
        ops.cfg_sampler_step_scaled(eps, x, None, mi, torch.ones(2, 2, device="cuda"), C.COEFFS["five"][:4] + (0.0,))
    with pytest.raises(ValueError, match="per=1"):
        ops.guidance_table(torch.zeros(2, 1, dtype=f16, device="cuda"), 1, 7.5, 0.5)
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_sampler_step_scaled(eps, x, None, mi, table, C.COEFFS["five"])
    ops.cfg_sampler_step_scaled(eps, x, None, mi, table, C.COEFFS["five"][:4] + (0.0,))


# ------------------------------------------------------------------ 4. the pipelines
STEPS = 4
PIPE_PHI = 0.7


@pytest.fixture(scope="module")
def small():
    import golden_util as G
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    from test_gpu_engine import SMALL_KW, build
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 11)
    return build(sd, **SMALL_KW), sd


@pytest.fixture(scope="module")
def small_vsr():
    from test_gpu_vsr import build_small_vsr
    return build_small_vsr()


def make_pipe(net, method):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    return VideoGenPipeline.from_sample_yaml(dict(sample_method=method), unet=net)[0]


def base_case(seed, frames, prompts=1):
    g = torch.Generator().manual_seed(seed)
    pe, ne = torch.randn(prompts, 77, 128, generator=g), torch.randn(prompts, 77, 128, generator=g)
    return pe, ne, torch.randn(prompts, 4, frames, 8, 8, generator=g)


def oracle_loop(sd, method, lat, pe, ne, guidance, phi, gen, window=None, known=None, mask=None, noise=None):
    """Test-side fp32 loop: the oracle UNet per window, guidance, rescale_noise_cfg (guidance_reference: the published formula) on
    every window's prediction, the windows averaged per frame with the exact normalised weights, the scheduler update written out
    from `coefficients`, the known-region replacement after the step."""
    import known_reference as K
    import window_reference as W
    from lavie_amd.windows import window_profile, window_starts
    from oracle import unet_fp32 as O
    from test_gpu_engine import ocfg_small
    sch = make_pipe(object(), method).scheduler
    sch.set_timesteps(STEPS)
    frac = bool(getattr(sch, "fractional_timesteps", False))
    ts = [float(t) if frac else int(t) for t in sch.timesteps]
    scale = getattr(sch, "model_input_scale", lambda t: 1.0)
    ctx = torch.cat([ne, pe]).half().float()
    frames = lat.shape[2]
    length, stride = window or (frames, frames)
    starts, profile = window_starts(frames, length, stride), window_profile(length, "triangle")
    weights = W.exact_weights(frames, starts, profile)
    x = lat * sch.init_noise_sigma
    if known is not None:
        a, s = sch.noise_level(ts[0])
        x = (1.0 - mask) * x + mask * (a * known + s * noise)
    x0_prev = None
    for i, t in enumerate(ts):
        fused = torch.zeros_like(x)
        for w, s in enumerate(starts):
            xin = (x[:, :, s:s + length] * scale(t)).half().float()
            e = O.unet_forward(sd, torch.cat([xin, xin]), t, ctx, ocfg_small())
            e = R.rescale_noise_cfg(e[:1] + guidance * (e[1:] - e[:1]), e[1:], phi)
            for f in range(s, s + length):
                fused[:, :, f] += weights[(w, f)] * e[:, :, f - s]
        k_x, k_e, c_x0, c_xt, c4 = sch.coefficients(t)
        x0 = k_x * x - k_e * fused
        if getattr(sch, "multistep", False):
            d = x0 + c4 * (x0 - x0_prev) if (c4 != 0.0 and i > 0) else x0
            x = c_xt * x + c_x0 * d
            x0_prev = x0 if mask is None else (1.0 - mask) * x0 + mask * known
        else:
            x = c_xt * x + c_x0 * x0
            if c4 != 0.0:
                x = x + c4 * torch.randn(x.shape, generator=gen)
        if known is not None:
            x = K.replace_known(x, known, mask, noise, sch.noise_level(ts[i + 1] if i + 1 < STEPS else None))
    return x


def check_against_oracle(label, out, ref, plain):
    from test_gpu_dpmsolver import TOL_PIPELINE
    err, moved = R.rel_l2(out, ref), R.rel_l2(out, plain)
    print(f"{label}: rel-L2 vs oracle loop {err:.3e}; moved {moved:.3e} from the run without rescale")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE
    assert moved > 0.0


@pytest.mark.parametrize("method", ["ddpm", "ddim", "dpmsolver++"])
def test_videogen_pipeline_with_rescale_vs_oracle_loop(small, method):
    net, sd = small
    pipe = make_pipe(net, method)
    pe, ne, lat = base_case(91, 8)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=64, video_length=8, num_inference_steps=STEPS,
              guidance_scale=7.5, output_type="latent", latents=lat)
    out = pipe(guidance_rescale=PIPE_PHI, generator=torch.Generator().manual_seed(3), **kw).video.float().cpu()
    plain = pipe(generator=torch.Generator().manual_seed(3), **kw).video.float().cpu()
    ref = oracle_loop(sd, method, lat, pe, ne, 7.5, PIPE_PHI, torch.Generator().manual_seed(3))
    check_against_oracle(f"{method} rescale {PIPE_PHI}", out, ref, plain)
    # guidance off: the keyword is ignored, as in diffusers
    off = dict(kw, guidance_scale=1.0)
    assert torch.equal(pipe(guidance_rescale=PIPE_PHI, generator=torch.Generator().manual_seed(3), **off).video,
                       pipe(generator=torch.Generator().manual_seed(3), **off).video)


def test_videogen_known_latents_and_windows_with_rescale_vs_oracle_loop(small):
    net, sd = small
    pipe = make_pipe(net, "ddim")
    pe, ne, lat = base_case(93, 8)
    g = torch.Generator().manual_seed(5)
    known, noise = torch.randn(1, 4, 8, 8, 8, generator=g) * 0.8, torch.randn(1, 4, 8, 8, 8, generator=g)
    mask = torch.zeros(1, 1, 8, 8, 8)
    mask[:, :, :2] = 1.0
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    kw = dict(known=known.cuda(), mask=mask, known_noise=noise.cuda())
    out = pipe.denoise(x_t, ctx, STEPS, 7.5, guidance_rescale=PIPE_PHI, **kw).float().cpu()
    plain = pipe.denoise(x_t, ctx, STEPS, 7.5, **kw).float().cpu()
    assert torch.equal(out[:, :, :2], known[:, :, :2])
    ref = oracle_loop(sd, "ddim", lat, pe, ne, 7.5, PIPE_PHI, None, known=known, mask=mask, noise=noise)
    check_against_oracle("ddim, 2 of 8 frames pinned", out, ref, plain)
    # 13 frames as two 8-frame windows at stride 6, DPM-Solver++
    pipe = make_pipe(net, "dpmsolver++")
    pe, ne, lat = base_case(95, 13)
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    out = pipe.denoise(x_t, ctx, STEPS, 7.5, window_length=8, window_stride=6, guidance_rescale=PIPE_PHI).float().cpu()
    plain = pipe.denoise(x_t, ctx, STEPS, 7.5, window_length=8, window_stride=6).float().cpu()
    ref = oracle_loop(sd, "dpmsolver++", lat, pe, ne, 7.5, PIPE_PHI, None, window=(8, 6))
    check_against_oracle("dpmsolver++, 13 frames as windows of 8 at stride 6", out, ref, plain)


@pytest.fixture
def one_split():
    """The GEMMs' automatic split-K factor depends on the batch, so a batch of two and two single calls do not give one forward's
    bits whatever the step does: measured with the scalar guidance 7.5 and the step kernel as it was, 3 DDIM steps at this shape,
    rel-L2 2.4e-3 / 2.6e-3 between the batched and the single runs, and 0 (bit-equal) with the factor pinned to 1."""
    from lavie_amd import _lib
    lib = _lib.load()
    assert lib.lavie_debug_force_splits(1) == 0
    yield
    lib.lavie_debug_force_splits(0)


def test_a_batched_call_with_a_scale_per_prompt_equals_two_single_calls(small, one_split):
    """Bit for bit, with the forward's split-K factor pinned (see `one_split`): table, statistics and step are per latent."""
    net, _ = small
    pipe = make_pipe(net, "ddim")
    pe, ne, lat = base_case(97, 4, prompts=2)
    kw = dict(height=64, width=64, video_length=4, num_inference_steps=3, output_type="latent")
    both = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=[5.0, 9.0], guidance_rescale=PIPE_PHI, **kw).video
    for q, g in enumerate((5.0, 9.0)):
        one = pipe(prompt_embeds=pe[q:q + 1], negative_prompt_embeds=ne[q:q + 1], latents=lat[q:q + 1], guidance_scale=g,
                   guidance_rescale=PIPE_PHI, **kw).video
        assert torch.equal(both[q:q + 1], one), q
    # without rescale a sequence still takes the table route; equal scales give the scalar route's bits
    seq = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=[7.5, 7.5], **kw).video
    assert torch.equal(seq, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5, **kw).video)
    with pytest.raises(ValueError, match="2 prompts"):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=[5.0], **kw)
    with pytest.raises(ValueError, match="> 1"):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=[5.0, 1.0], **kw)
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5, guidance_rescale=1.2, **kw)


def test_vsr_pipeline_with_rescale_vs_oracle_loop(small_vsr):
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.vsr import VideoUpscalePipeline
    from oracle import vsr_blocks as V
    from oracle.ddim import DDIMSchedule
    from oracle.vsr_loop import add_low_res_noise
    net, sd = small_vsr
    pipe = VideoUpscalePipeline(unet=net, scheduler=DDIMScheduler())
    g = torch.Generator().manual_seed(77)
    pe, ne = torch.randn(1, 77, 128, generator=g).half().float(), torch.randn(1, 77, 128, generator=g).half().float()
    frames, lat = torch.randn(1, 3, 4, 8, 8, generator=g).clamp(-1, 1), torch.randn(1, 4, 4, 8, 8, generator=g)
    kw = dict(image=frames, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=9.0,
              noise_level=20)
    out = pipe(guidance_rescale=PIPE_PHI, generator=torch.Generator().manual_seed(5), **kw).images.float().cpu()
    plain = pipe(generator=torch.Generator().manual_seed(5), **kw).images.float().cpu()
    img = add_low_res_noise(frames, torch.randn(frames.shape, generator=torch.Generator().manual_seed(5)), 20)
    sch = DDIMSchedule()
    sch.set_timesteps(3)
    ctx, low, labels = torch.cat([ne, pe]), torch.cat([img, img]), torch.full((2,), 20, dtype=torch.long)
    x = lat
    for t in sch.timesteps:
        eps = V.vsr_unet_forward(sd, torch.cat([x, x]), low, t, ctx, labels, block_out_channels=(256, 512), attn_levels=(False, True),
                                 only_cross_attention=(True, False), layers_per_block=1, heads=8)
        e_u, e_c = eps.chunk(2)
        x = sch.step(R.rescale_noise_cfg(e_u + 9.0 * (e_c - e_u), e_c, PIPE_PHI), t, x, eta=0.0, noise=None)
    check_against_oracle("vsr ddim", out, x, plain)
