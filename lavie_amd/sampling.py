"""The denoising loop of this package, once.  `Run` holds what a loop over one clip owns (fp32 latents, window geometry, one fp16
model input per window, x0 history, step noise, the current step plan, guidance, known region, layer-cache interval, FreeInit
state), fills the model inputs (`Run.fill`) and runs the FreeInit iterations and their steps (`Run.loop`).  `check_features` judges
which sampling features a call combines, from the one table `REFUSED`.  Beside them the pieces a loop is made of, each once: the
step plan, the step's noise (four generator kinds, host draws staged through pinned memory), the engine and layer-cache sessions,
the guidance arguments and the per-latent guidance table, the choice among the fused step ops, the forwards of a windowed step.
A pipeline (`VideoGenPipeline.denoise`, `VideoUpscalePipeline.denoise`) says only what is its own: which tensors reach the UNet
(`forward(w, i, layer_cache_mode)`), the sessions around the loop and their order, and its checks of its own arguments.
`SpacedDiffusion._ddim_loop_hip` keeps its own schedule and arithmetic and takes the engine session only."""
import contextlib
import inspect
import math
import os
import sys

from collections import namedtuple

import torch

from . import free_init as free_init_mod
from . import _lib, ops, windows
from .noise import NoiseKey, PhiloxGenerator
from .scheduling_ddpm import randn_tensor


class StepPlan:
    """The timesteps of `scheduler` at `num_inference_steps` and the scalars of step i (a position in `timesteps`)."""

    def __init__(self, scheduler, num_inference_steps: int, eta: float = 0.0):
        scheduler.set_timesteps(num_inference_steps)
        # Euler's timesteps are fractional (linspace) and reach the UNet as they are; DDPM / DDIM timesteps are integers
        fractional = bool(getattr(scheduler, "fractional_timesteps", False))
        self.timesteps = [float(t) if fractional else int(t) for t in scheduler.timesteps]
        # a multistep scheduler says so itself (DPMSolverMultistepScheduler.multistep): its fifth coefficient is c_prev, not a
        # noise sigma, and the step kernel keeps the previous x0 prediction in a buffer beside the fp32 latents
        self.multistep = bool(getattr(scheduler, "multistep", False))
        # UniPCMultistepScheduler says `unipc`: its `coefficients` are the ten scalars of the predictor-corrector step kernel, which
        # keeps the previous corrected sample and two x0 predictions in three buffers beside the fp32 latents
        self.unipc = bool(getattr(scheduler, "unipc", False))
        self._scheduler = scheduler
        # `eta` goes to the scheduler only if its step takes one (DDIM), as prepare_extra_step_kwargs does
        # (pipeline_videogen.py:431-446); DDPM ignores it
        self._eta = (eta,) if "eta" in inspect.signature(scheduler.coefficients).parameters else ()
        # scheduler.scale_model_input (pipeline_videogen.py:667) as a scalar the fused kernel applies to the fp16 model input
        self._in_scale = getattr(scheduler, "model_input_scale", None)

    def t_dev(self, device) -> torch.Tensor:
        return torch.tensor(self.timesteps, dtype=torch.float32, device=device)

    def coeffs(self, i: int, first: bool = False):
        """The scheduler's five coefficients of step i.  `first`: the run starts at this step, so a multistep scheduler has no
        x0 history yet and the step is first order (c_prev = 0; at position 0 the scheduler says so itself)."""
        c = self._scheduler.coefficients(self.timesteps[i], *self._eta)
        return tuple(c[:4]) + (0.0,) if first and self.multistep else c

    def adds_noise(self, coeffs) -> bool:
        """DDPM: every step but the last; DDIM: only with eta > 0; a multistep scheduler's fifth coefficient is no sigma."""
        return not self.multistep and not self.unipc and coeffs[4] != 0.0

    def input_scale(self, i: int) -> float:
        """Scale of the model input of step i; 1.0 without `model_input_scale` or past the last step."""
        return self._in_scale(self.timesteps[i]) if self._in_scale and i < len(self.timesteps) else 1.0

    def noise_level(self, i_next: int):
        """(a, s) the known latents are re-noised with after the step in front of position `i_next`: (1, 0) past the end."""
        return self._scheduler.noise_level(self.timesteps[i_next] if i_next < len(self.timesteps) else None)


# device -> the one copy stream of every StepNoise on that device, for the life of the process.  Shared on purpose: a loop keeps
# no stream of its own, so a pipeline call does not start on a stream the runtime has never submitted to.  Safe because nothing
# relies on the stream's identity: each slot's copy is ordered behind that slot's last consumer and in front of its next one by
# events that belong to the StepNoise object, so two objects on one stream can only wait for each other, never read each other.
_side_streams = {}


class SeededNoise:
    """What `StepNoise.draw()` hands the loop for a `noise.PhiloxGenerator`: the step's key, not a tensor.  `step` / `window_step`
    pass `key` to a fused seeded step where one exists; for the others `tensor()` materialises the same values (ops.philox_normal)
    into the one buffer the StepNoise allocates on first use and keeps for the run."""

    def __init__(self, key: NoiseKey, owner):
        self.key, self._owner = key, owner

    def tensor(self) -> torch.Tensor:
        return self._owner.materialise(self.key)


class StepNoise:
    """Per-step fp32 noise shaped as `x`, on x's device, from `generator`: None, one generator or one per latent (as
    randn_tensor takes them, :504), on the host or the device.  Host draws for a device tensor are staged through two pinned
    slots on a side stream so that neither the device nor the host waits for the other: `draw()` makes the main stream wait
    for the slot's copy, `done()` after the consuming launch lets the side stream overwrite the slot two draws later.
    A `noise.PhiloxGenerator`: `draw()` hands out a SeededNoise (the key of the draw); there are no buffers, no side stream and no
    events, and nothing is allocated unless a step without a fused seeded form asks for the tensor."""

    def __init__(self, x: torch.Tensor, generator=None):
        self._philox = generator if isinstance(generator, PhiloxGenerator) else None
        if self._philox is not None:
            self._shape, self._device, self._buffer = tuple(x.shape), x.device, None
            self._philox.seeds(x.shape[0])          # a seed list of another length is refused here, in front of the loop
            self._staged, self._pending = False, None
            return
        self._per_latent = isinstance(generator, list)
        self._gens = generator if self._per_latent else [generator]
        if self._per_latent:
            if len(self._gens) != x.shape[0]:
                raise ValueError(f"got a list of {len(self._gens)} generators for {x.shape[0]} latents")
            if len({g.device.type for g in self._gens}) != 1:
                raise ValueError("a list of generators must live on one device type")
        self._staged = x.is_cuda and self._gens[0] is not None and self._gens[0].device.type == "cpu"
        self._pending = None            # the slot whose consumer has not been launched yet
        if not self._staged:            # drawn where x lives
            self._noise = torch.empty_like(x)
            return
        self._pinned = [torch.empty(x.shape, dtype=torch.float32).pin_memory() for _ in range(2)]
        self._noise = [torch.empty_like(x) for _ in range(2)]
        self._copy_done = [None, None]  # slot's H2D copy finished  -> host may refill the pinned slot
        self._step_done = [None, None]  # slot's consumer finished  -> side stream may overwrite the device slot
        if x.device not in _side_streams:
            _side_streams[x.device] = torch.cuda.Stream(device=x.device)
        self._side = _side_streams[x.device]
        self._main = torch.cuda.current_stream(x.device)
        self._draws = 0

    def _fill(self, out):
        if self._per_latent:
            for j, g in enumerate(self._gens):
                out[j].normal_(generator=g)
        else:
            out.normal_(generator=self._gens[0])
        return out

    def materialise(self, key: NoiseKey) -> torch.Tensor:
        """The tensor of a seeded draw, in the run's one buffer."""
        if self._buffer is None:
            self._buffer = torch.empty(self._shape, dtype=torch.float32, device=self._device)
        ops.philox_normal(key.seeds, math.prod(self._shape[1:]), key.draw, out=self._buffer)
        return self._buffer

    def draw(self):
        if self._philox is not None:
            return SeededNoise(self._philox.key(self._shape[0]), self)
        if not self._staged:
            return self._fill(self._noise)
        slot = self._draws & 1
        self._draws += 1
        if self._copy_done[slot] is not None:
            self._copy_done[slot].synchronize()
        self._fill(self._pinned[slot])
        if self._step_done[slot] is not None:
            self._side.wait_event(self._step_done[slot])
        with torch.cuda.stream(self._side):
            self._noise[slot].copy_(self._pinned[slot], non_blocking=True)
        self._copy_done[slot] = torch.cuda.Event()
        self._copy_done[slot].record(self._side)
        self._main.wait_event(self._copy_done[slot])
        self._pending = slot
        return self._noise[slot]

    def done(self):
        """Call after the launch that consumed the last `draw()` (harmless when the step drew none)."""
        if self._pending is not None:
            self._step_done[self._pending] = torch.cuda.Event()
            self._step_done[self._pending].record(self._main)
            self._pending = None


@contextlib.contextmanager
def engine_session(unet, batch: int, frames: int, height: int, width: int, ctx: torch.Tensor, shared_inputs=None):
    """The engine prepared for [batch, C, frames, height, width] with `ctx` cached for the whole loop (its keys / values are
    computed once; the reference recomputes them in each block of each step, attention.py:177-178); yields the context to pass
    to the UNet.  `shared_inputs`: the loop's fp16 model inputs when both CFG halves of each hold the same latents (written by
    the loop's own step kernel), so the engine may compute the layers in front of the first text cross-attention once;
    LAVIE_DEBUG_CHECK_SHARED=1 checks every one of them.  A UNet without `cache_context` / `set_cfg_shared_input` runs without.
    On exit the engine lets go of both, also after an exception in the loop, which clean-up never masks: each undo is attempted
    and a failure of its own is re-raised only when the loop itself finished."""
    unet.prepare(batch, frames, height, width, ctx.shape[1])
    caches = hasattr(unet, "cache_context")
    if caches:
        ctx = unet.cache_context(ctx)
    shared = shared_inputs is not None and hasattr(unet, "set_cfg_shared_input")
    try:
        if shared:
            unet.set_cfg_shared_input(True)
            if os.environ.get("LAVIE_DEBUG_CHECK_SHARED") == "1":
                for m in shared_inputs:
                    if not torch.equal(m[:m.shape[0] // 2], m[m.shape[0] // 2:]):
                        raise RuntimeError("cfg_shared_prefix: the two halves of the model input differ")
        yield ctx
    finally:
        pending = sys.exc_info()[1]
        cleanup_error = None
        for undo in ((lambda: unet.set_cfg_shared_input(False)) if shared else None,
                     (lambda: unet.cache_context(None)) if caches else None):
            if undo is None:
                continue
            try:
                undo()
            except Exception as e:      # noqa: BLE001
                cleanup_error = cleanup_error or e
        if cleanup_error is not None and pending is None:
            raise cleanup_error


def check_layer_cache(cache_interval, cache_depth=1, windowed: bool = False) -> int:
    """The layer-cache arguments of a pipeline call -> the interval in force: 1 = off (`cache_interval` None or 1: the call without
    it), N > 1 = the whole UNet runs on every N-th executed step and the shallow walk on the steps between (`layer_cache_mode`).
    Not combined with frame windows: a windowed step runs several forwards, each of which would need a cache of its own."""
    if cache_interval is None:
        return 1
    if isinstance(cache_interval, bool) or not isinstance(cache_interval, int) or cache_interval < 1:
        raise ValueError(f"`cache_interval` must be an integer >= 1 (or None) but is {cache_interval!r}")
    if isinstance(cache_depth, bool) or not isinstance(cache_depth, int) or cache_depth < 1:
        raise ValueError(f"`cache_depth` must be an integer >= 1 but is {cache_depth!r}")
    if cache_interval > 1 and windowed:
        raise ValueError(REFUSED["cache", "windowed"])
    return cache_interval


def layer_cache_mode(executed: int, cache_interval: int):
    """The `layer_cache` argument of the UNet forward of the `executed`-th step a loop runs (0 = its first, wherever in the timestep
    table it starts): None without caching, "refresh" iff executed % cache_interval == 0, else "reuse"."""
    if cache_interval <= 1:
        return None
    return "refresh" if executed % cache_interval == 0 else "reuse"


@contextlib.contextmanager
def layer_cache_session(unet, cache_interval: int, cache_depth: int = 1):
    """The UNet's layer cache switched on at `cache_depth` for one loop (cache_interval > 1) and put back to the model's own setting
    afterwards, also after an exception; what the loop cached is dropped either way.  cache_interval <= 1: nothing is touched."""
    if cache_interval <= 1:
        yield
        return
    if not hasattr(unet, "enable_layer_cache"):
        raise ValueError(f"`cache_interval` > 1: {type(unet).__name__} has no layer cache")
    was = unet.layer_cache
    unet.enable_layer_cache(cache_depth)
    try:
        yield
    finally:
        if was:
            unet.enable_layer_cache(was)
        else:
            unet.disable_layer_cache()


def check_guidance(guidance_scale, guidance_rescale, count: int, repeat: int = 1):
    """The guidance arguments of a pipeline call -> (guided, scales, rescale).  `guidance_scale`: one number (guidance is on when
    it is > 1), or a sequence with one value for each of the `count` prompts, every one > 1 (a sequence always means guidance is
    on), as a list, a tuple or a tensor of one dimension or more; `scales` is then the list with every value repeated `repeat`
    times (latents are prompt-major), else None.
    `guidance_rescale` = phi in [0, 1] (Lin et al., diffusers' rescale_noise_cfg); without guidance it is ignored, as in
    diffusers, and comes back as 0."""
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"`guidance_rescale` must lie in [0, 1] but is {guidance_rescale}")
    if isinstance(guidance_scale, torch.Tensor) and guidance_scale.dim() > 0:      # a 0-dim tensor is one number, as it always was
        guidance_scale = guidance_scale.flatten().tolist()
    if isinstance(guidance_scale, (list, tuple)):
        scales = [float(v) for v in guidance_scale]
        if len(scales) != count:
            raise ValueError(f"`guidance_scale` has {len(scales)} values for {count} prompts")
        if not all(v > 1.0 for v in scales):
            raise ValueError(f"every value of a `guidance_scale` sequence must be > 1, got {scales}")
        return True, [v for v in scales for _ in range(int(repeat))], phi
    guided = guidance_scale > 1.0
    return guided, None, phi if guided else 0.0


class GuidanceTable:
    """The table route of a guided loop: guidance scales per latent (`scales`: a list, or one number) and / or guidance rescale
    (`rescale` > 0).  Holds what `ops.guidance_table` needs, allocated once per loop beside the noise buffers: the scales on the
    device, the partial-sum workspace and the table itself, [P, 2] or, for `windows` > 1 forwards per step, [W, P, 2] with `per`
    the elements of one latent of one forward.  Calling it with the step's predictions enqueues the table's two launches."""

    def __init__(self, scales, rescale: float, latents: int, per: int, device, windows: int = 1):
        self.latents, self.rescale, self.windowed = int(latents), float(rescale), windows > 1
        self.scales = torch.tensor(scales, dtype=torch.float32, device=device) if isinstance(scales, (list, tuple)) else float(scales)
        self.table = torch.empty(((windows,) if self.windowed else ()) + (self.latents, 2), dtype=torch.float32, device=device)
        self.workspace = torch.empty(ops.guidance_partials_floats(windows * self.latents, per), dtype=torch.float32,
                                     device=device) if self.rescale != 0.0 else None

    def __call__(self, eps: list) -> torch.Tensor:
        return ops.guidance_table(eps if self.windowed else eps[0], self.latents, self.scales, self.rescale, self.workspace,
                                  self.table)


def guidance_of(guidance_scale, guidance_rescale, x: torch.Tensor, frames: int, windows: int = 1):
    """What a loop over latents x [P, C, F, h, w] hands to `step` / `window_step` as guidance: None (no guidance), the scalar
    `guidance_scale` itself (today's launches), or a GuidanceTable when `guidance_rescale` > 0 or `guidance_scale` is a sequence
    with one value per latent.  `frames`: frames of one forward."""
    guided, scales, phi = check_guidance(guidance_scale, guidance_rescale, x.shape[0])
    if not guided:
        return None
    if scales is None and phi == 0.0:
        return guidance_scale
    per = x.shape[1] * frames * math.prod(x.shape[3:])
    return GuidanceTable(scales if scales is not None else guidance_scale, phi, x.shape[0], per, x.device, windows)


class PagGuidance:
    """The guidance of a step with perturbed-attention guidance: `guidance_scale` (a number, or None without classifier-free
    guidance) and the step's PAG scale, which the loop sets before each step (`pag_scale_at`)."""

    def __init__(self, guidance_scale, pag_scale: float):
        self.guidance_scale, self.pag_scale = guidance_scale, float(pag_scale)


def pag_scale_at(pag_scale: float, pag_adaptive_scale: float, timestep) -> float:
    """The PAG scale of the step at `timestep`: max(pag_scale - pag_adaptive_scale (1000 - t), 0), diffusers' _get_pag_scale (the
    scale fades as sampling proceeds when pag_adaptive_scale > 0)."""
    return max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(timestep)), 0.0)


def check_pag_scales(pag_scale, pag_adaptive_scale) -> bool:
    """The two numbers of perturbed-attention guidance -> whether it is on (pag_scale > 0)."""
    pag_scale, pag_adaptive_scale = float(pag_scale), float(pag_adaptive_scale)
    if not (pag_scale >= 0.0 and pag_scale != float("inf")):
        raise ValueError(f"`pag_scale` must be finite and >= 0 but is {pag_scale}")
    if not (pag_adaptive_scale >= 0.0 and pag_adaptive_scale != float("inf")):
        raise ValueError(f"`pag_adaptive_scale` must be finite and >= 0 but is {pag_adaptive_scale}")
    return pag_scale > 0.0


# Which sampling features are not combined: (feature, what it refuses) -> the refusal.  One feature's rows are judged in the order
# they stand here.  `known`: any known-latents argument, a late start or reduced strength among them; `argument`: a known-latents
# tensor or `window_length` is given (what PAG refuses, naming the first, {argument}); `window_length`: that argument is given;
# `windowed`: it is below the clip's length, so windows are in force.  {known} / {free_init} are the caller's words (`Surface`).
REFUSED = {
    ("free_init", "known"): "{free_init} cannot be combined with {known}: the run's start is not noise there",
    ("cache", "windowed"): "`cache_interval` > 1 cannot be combined with frame windows (`window_length`): every window's forward "
                           "would need a layer cache of its own",
    ("pag", "argument"): "`pag_scale` > 0 cannot be combined with `{argument}`",
    ("pag", "sequence"): "`pag_scale` > 0 cannot be combined with a `guidance_scale` sequence (one value per prompt)",
    ("pag", "rescale"): "`pag_scale` > 0 cannot be combined with `guidance_rescale` > 0",
    ("window_length", "known"): "frame windows (`window_length`) cannot be combined with {known}",
    # the UniPC sampler (`unipc`: the call's scheduler is a UniPCMultistepScheduler), judged in front of every other feature
    ("unipc", "known"): "the UniPC sampler (UniPCMultistepScheduler) cannot be combined with {known}: its step kernel has no "
                        "known-region form and a run that starts late has no history",
    ("unipc", "window_length"): "the UniPC sampler (UniPCMultistepScheduler) cannot be combined with frame windows (`window_length`)",
    ("unipc", "pag"): "the UniPC sampler (UniPCMultistepScheduler) cannot be combined with `pag_scale` > 0",
    ("unipc", "free_init"): "the UniPC sampler (UniPCMultistepScheduler) cannot be combined with {free_init}",
}

# How one caller of `check_features` speaks: the features it judges, in the order it has always judged them (of two refusals that
# apply to one call the earlier feature's is raised), and its words for FreeInit and for the known-latents arguments in a refusal.
Surface = namedtuple("Surface", "order free_init known", defaults=("", ""))


def check_features(surface, clip_frames: int, prompts: int = 0, known=None, late_start: bool = False, window_length=None,
                   guidance=(1.0, 0.0), pag=(0.0, 0.0), cache=(None, 1), free_init=None, unipc: bool = False):
    """The sampling features of one call on a clip of `clip_frames` frames and `prompts` latents, as far as `surface.order` names
    them: each feature's own arguments through its validator, then every pair of `REFUSED` that the call combines refused ->
    (the FreeInit setting or None, the layer-cache interval in force, whether PAG is on).  A feature outside the order is neither
    validated nor refused and comes back as off.  known: the caller's known-latents tensors by argument name (None = absent);
    late_start: the run starts past position 0 or below full strength; guidance = (guidance_scale, guidance_rescale), looked at
    only for PAG's rows (`check_guidance` stays where each caller has it); pag = (pag_scale, pag_adaptive_scale); cache =
    (cache_interval, cache_depth).  unipc: the call samples with UniPC, which claims guidance, the guidance table, the layer cache and
    seeded initial latents only; every other feature the call asks for is refused first, whatever the surface's order.  Raises
    before anything reaches the engine."""
    if unipc:
        asked = {"known": late_start or any(value is not None for value in (known or {}).values()),
                 "window_length": window_length is not None, "pag": float(pag[0]) > 0.0,
                 "free_init": free_init_mod.coerce(free_init) is not None}
        for what, is_on in asked.items():
            if is_on:
                raise ValueError(REFUSED["unipc", what].format(free_init=surface.free_init or "FreeInit (`free_init`)",
                                                               known=surface.known or "known latents"))
    given = dict(known or {})
    given.setdefault("window_length", window_length)
    argument = next((name for name, value in given.items() if value is not None), None)
    scale, rescale = guidance
    on = {"argument": argument is not None, "known": late_start or any(value is not None for value in (known or {}).values()),
          "window_length": window_length is not None, "windowed": window_length is not None and clip_frames > int(window_length),
          "sequence": isinstance(scale, (list, tuple)) or (isinstance(scale, torch.Tensor) and scale.dim() > 0),
          "rescale": "pag" in surface.order and float(rescale) > 0.0, "pag": False}
    free, interval = None, 1
    for feature in surface.order:
        if feature == "free_init":
            free = free_init_mod.coerce(free_init)
            on[feature] = free is not None
        elif feature == "cache":
            interval = check_layer_cache(*cache)
            on[feature] = interval > 1
        elif feature == "pag":
            on[feature] = check_pag_scales(*pag)
        for (first, second), text in REFUSED.items():
            if first == feature and on[first] and on[second]:
                raise ValueError(text.format(free_init=surface.free_init, known=surface.known, argument=argument))
        if feature == "pag" and on["pag"]:                  # the engine's batch limit of 8
            guided = scale > 1.0
            most, parts = (2, "[negative | prompt | perturbed]") if guided else (4, "[prompt | perturbed]")
            if prompts > most:
                raise ValueError(f"`pag_scale` > 0 serves at most {most} prompts per call {'with' if guided else 'without'} guidance "
                                 f"(the engine's batch limit of 8 holds {parts}), got {prompts}")
    return free, interval, on["pag"]


def step(eps, x, aux, model_in, guidance_scale, coeffs, next_scale, multistep: bool, region=None):
    """One fused scheduler step through the `ops` wrapper of its family.  `aux`: the step's noise or None (five-coefficient
    family), the x0 history (multistep).  `guidance_scale` None: no classifier-free guidance; a GuidanceTable: the table is
    computed from `eps` and the `_scaled` wrapper of the family reads it.  `region`: None, or (known, mask, known_noise, level) of
    a run around known latents.  A PagGuidance: eps / model_in hold the perturbed part as well and the `pag` wrappers run.  The
    wrappers are looked up on `ops` at call time."""
    if isinstance(guidance_scale, PagGuidance):
        if region is not None:
            raise ValueError("perturbed-attention guidance is not combined with a known region")
        g = guidance_scale.guidance_scale
        kind, guidance = ("pag_cfg", (g, guidance_scale.pag_scale)) if g is not None else ("pag", (guidance_scale.pag_scale,))
    elif isinstance(guidance_scale, GuidanceTable):
        kind, guidance = "table", (guidance_scale([eps]),)
    else:
        kind, guidance = ("scalar", (guidance_scale,)) if guidance_scale is not None else ("none", ())
    if isinstance(aux, SeededNoise):            # seeded engine noise: the key where a fused form exists, else the materialised tensor
        if kind in STEP_SEEDED and region is None and not multistep and x.shape[0] <= _lib.NOISE_MAX_SEEDS:
            getattr(ops, STEP_SEEDED[kind])(eps, x, aux.key, model_in, *guidance, coeffs, next_scale)
            return
        aux = aux.tensor()
    name = STEP_WRAPPERS[bool(multistep), kind, region is not None]
    getattr(ops, name)(eps, x, aux, model_in, *guidance, coeffs, next_scale, *(region or ()))


def unipc_step(eps, x, history, model_in, guidance_scale, coeffs, next_scale):
    """One fused UniPC step through its `ops` wrapper.  `history`: the run's (x_last, m1, m2).  `guidance_scale` as in `step`:
    None, a number, or a GuidanceTable (computed from `eps` first); nothing else is combined with this sampler."""
    if isinstance(guidance_scale, GuidanceTable):
        kind, guidance = "table", (guidance_scale([eps]),)
    elif isinstance(guidance_scale, PagGuidance):
        raise ValueError(REFUSED["unipc", "pag"])
    else:
        kind, guidance = ("scalar", (guidance_scale,)) if guidance_scale is not None else ("none", ())
    getattr(ops, UNIPC_WRAPPERS[kind])(eps, x, history, model_in, *guidance, coeffs, next_scale)


# guidance kind -> the `ops` wrapper of `unipc_step`
UNIPC_WRAPPERS = {"none": "unipc_step", "scalar": "cfg_unipc_step", "table": "cfg_unipc_step_scaled"}

# guidance kind -> the `ops` wrapper of a plain five-coefficient step that makes its noise from a key (no region, no table, no PAG)
STEP_SEEDED = {"none": "sampler_step_seeded", "scalar": "cfg_sampler_step_seeded"}

# (multistep, guidance kind, region) -> the `ops` wrapper of `step`
STEP_WRAPPERS = {
    (False, "none", False): "sampler_step",                 (False, "none", True): "sampler_step_known",
    (False, "scalar", False): "cfg_ddpm_step",              (False, "scalar", True): "cfg_sampler_step_known",     # lines 667, 679-683 fused
    (False, "table", False): "cfg_sampler_step_scaled",     (False, "table", True): "cfg_sampler_step_known_scaled",
    (True, "none", False): "multistep_step",                (True, "none", True): "multistep_step_known",
    (True, "scalar", False): "cfg_multistep_step",          (True, "scalar", True): "cfg_multistep_step_known",
    (True, "table", False): "cfg_multistep_step_scaled",    (True, "table", True): "cfg_multistep_step_known_scaled",
    # perturbed-attention guidance, with and without classifier-free guidance (no region form)
    (False, "pag", False): "pag_sampler_step",              (False, "pag_cfg", False): "cfg_pag_sampler_step",
    (True, "pag", False): "pag_multistep_step",             (True, "pag_cfg", False): "cfg_pag_multistep_step",
}


def window_step(eps, x, aux, model_in, starts, profile, guidance_scale, coeffs, next_scale, multistep: bool):
    """One fused step over frame windows: `ops.window_step`, or with a GuidanceTable one `ops.guidance_table` call over all
    windows' predictions followed by `ops.window_step_scaled`.  A SeededNoise as `aux`: `ops.window_step_seeded` takes its key; under
    a GuidanceTable the tensor is materialised."""
    if isinstance(aux, SeededNoise):
        if not isinstance(guidance_scale, GuidanceTable) and not multistep and x.shape[0] <= _lib.NOISE_MAX_SEEDS:
            ops.window_step_seeded(eps, x, aux.key, model_in, starts, profile, guidance_scale, coeffs, next_scale)
            return
        aux = aux.tensor()
    if isinstance(guidance_scale, GuidanceTable):
        ops.window_step_scaled(eps, x, aux, model_in, starts, profile, guidance_scale(eps), coeffs, next_scale, multistep=multistep)
    else:
        ops.window_step(eps, x, aux, model_in, starts, profile, guidance_scale, coeffs, next_scale, multistep=multistep)


class WindowForwards:
    """The W noise predictions of one windowed step, all alive until the step kernel has read them.  `forward(w, i)` runs the
    UNet on window w at step i.  A UNet that hands back one buffer per shape (enable_graph) needs copies; whether it does is
    unknown until two forwards of one step have been seen."""

    def __init__(self, forward):
        self._forward = forward
        self._reuses_output = None      # None = not decided yet

    def __call__(self, count: int, i: int) -> list:
        eps = []
        for w in range(count):
            e = self._forward(w, i)
            if self._reuses_output is None and w == 1:
                self._reuses_output = e.data_ptr() == eps[0].data_ptr()
                if self._reuses_output:     # the second forward has overwritten the first prediction: redo that one
                    e = e.clone()
                    eps[0] = self._forward(0, i).clone()
            elif self._reuses_output:
                e = e.clone()
            eps.append(e)
        return eps


# Which frames each UNet forward of a step sees: `frames` per forward, the windows' first frames, the weight profile of one window
# (None without windows) and whether windows are in force.
Windows = namedtuple("Windows", "frames starts profile windowed")


def window_geometry(clip_frames: int, window_length=None, window_stride=None, window_weights: str = "triangle"):
    """The windows of a clip of `clip_frames` frames (lavie_amd.windows).  `window_length` None or not below the clip's length: one
    forward sees the whole clip.  `window_stride` defaults to three quarters of the window."""
    frames = clip_frames if window_length is None else int(window_length)
    if window_length is not None and frames < 1:
        raise ValueError(f"`window_length`={window_length} must be >= 1")
    if clip_frames <= frames:
        return Windows(clip_frames, [0], None, False)
    starts = windows.window_starts(clip_frames, frames, int(window_stride) if window_stride is not None else max(1, frames - frames // 4))
    return Windows(frames, starts, windows.window_profile(frames, window_weights), True)


class Run:
    """What a denoising loop over one clip owns, allocated once in front of the loop, and the loop itself.
    latents [P, C, F, h, w] (copied to fp32 `x`); `geometry`: the clip's Windows; `plan`: the StepPlan of the first (or only)
    iteration; `guidance`: what `guidance_of` made for this clip and geometry (None, the scalar, or a GuidanceTable); `batch`: the
    model batch, P times the parts [negative |] prompt [| perturbed]; `generator`: of the steps' noise and of `known_noise` when
    that is drawn here; pag: None or (pag_scale, pag_adaptive_scale); known: None or (known, mask, known_noise, start_step), the
    known region of `VideoGenPipeline.denoise`; `cache_interval`: the layer cache's, 1 = off.  `free`: None, or the FreeInitRun a
    pipeline with FreeInit sets once `x` exists; it also makes the plans of the later iterations."""

    def __init__(self, latents, geometry, plan: StepPlan, guidance, batch: int, generator=None, pag=None, known=None,
                 cache_interval: int = 1):
        self.x = x = latents.to(torch.float32).contiguous().clone()
        self.frames, self.starts, self.profile, self.windowed = geometry
        self.plan, self.batch, self.pag, self.cache_interval, self.free = plan, batch, pag, cache_interval, None
        self.guided = guidance is not None
        self.guidance = PagGuidance(guidance, pag[0]) if pag else guidance
        self.start_step, self.region = 0, None
        if known is not None:
            known, mask, known_noise, self.start_step = known
            if tuple(known.shape) != tuple(x.shape):
                raise ValueError(f"`known` has shape {tuple(known.shape)}, the latents {tuple(x.shape)}")
            if mask is not None:
                mask = mask.to(device=x.device, dtype=torch.float32).expand(x.shape[0], 1, *x.shape[2:]).contiguous()
        self.noise = StepNoise(x, generator)
        if known is not None:
            if known_noise is None:
                known_noise = randn_tensor(tuple(x.shape), generator=generator, device=x.device, dtype=torch.float32)
            elif tuple(known_noise.shape) != tuple(x.shape):
                raise ValueError(f"`known_noise` has shape {tuple(known_noise.shape)}, the latents {tuple(x.shape)}")
            self.region = tuple(None if t is None else t.to(device=x.device, dtype=torch.float32).contiguous()
                                for t in (known, mask, known_noise))
        self.x0_prev = torch.empty_like(x) if plan.multistep else None     # never read before the first step has written it (c_prev = 0)
        # UniPC: (x_last, m1, m2), none of them read before a step has written it; a Run is one chunk, one clip, one call, so every
        # one of them starts with a fresh history: position 0 has no corrector and a first-order predictor
        self.unipc_history = tuple(torch.empty_like(x) for _ in range(3)) if plan.unipc else None
        if plan.unipc and (self.windowed or pag or known is not None):
            what = "window_length" if self.windowed else "pag" if pag else "known"
            raise ValueError(REFUSED["unipc", what].format(known="known latents", free_init="FreeInit"))
        self.model_in = [torch.empty((self.batch, x.shape[1], self.frames) + tuple(x.shape[3:]), dtype=torch.float16, device=x.device)
                         for _ in self.starts]
        self.t_dev = plan.t_dev(x.device)

    def fill(self, scale: float):
        """Every model input from x at `scale`, as the step kernel leaves it: at the start of a run (around known latents x is
        first blended with them at the start position's noise level) and, with windows, after a FreeInit mix."""
        x, model_in = self.x, self.model_in
        if self.region is not None:
            known, mask, known_noise = self.region
            ops.known_blend(x, model_in[0], known, mask if self.start_step == 0 else None, known_noise,
                            self.plan.noise_level(self.start_step), scale)
        elif self.pag:                                      # one fp16 value in every part
            for part in model_in[0].view(self.batch // x.shape[0], -1):
                ops.latents_to_model_input1(x, part, scale)
        else:
            to_input = ops.latents_to_model_input if self.guided else ops.latents_to_model_input1
            for s, m in zip(self.starts, model_in):
                to_input(x[:, :, s:s + self.frames].contiguous(), m, scale)

    def loop(self, forward, callback=None, callback_steps: int = 1) -> torch.Tensor:
        """The FreeInit iterations (one without) and the steps of each, inside the caller's sessions -> x.  `forward(w, i,
        layer_cache_mode)` runs the UNet on `model_in[w]` at `t_dev[i]` and hands back its prediction; the mode is None without
        the layer cache (`forward_keywords`).  `callback(i, t, x)` after every `callback_steps`-th position."""
        x, model_in, noise, guidance, start = self.x, self.model_in, self.noise, self.guidance, self.start_step
        plan, masked, interval = self.plan, self.region is not None and self.region[1] is not None, self.cache_interval
        forwards = WindowForwards(lambda w, i: forward(w, i, layer_cache_mode(i - start, interval)))
        region = None
        if plan.unipc and self.free is not None:
            raise ValueError(REFUSED["unipc", "free_init"].format(free_init="FreeInit (`free_init`)"))
        for iteration in range(self.free.setting.num_iters if self.free is not None else 1):
            if iteration > 0:
                # the next iteration's plan first: its first input scale goes into the mix, which leaves x and, without windows,
                # every part of the model input as a step would (windows: cut from the mixed clip as at a run's start)
                self.plan = plan = self.free.plan_at(iteration)
                self.t_dev = plan.t_dev(x.device)
                self.free.remix(x, None if self.windowed else model_in[0], plan.input_scale(0))
                if self.windowed:
                    self.fill(plan.input_scale(0))
            for i in range(start, len(plan.timesteps)):
                eps = forwards(len(model_in), i)
                if self.pag:
                    guidance.pag_scale = pag_scale_at(*self.pag, plan.timesteps[i])
                coeffs = plan.coeffs(i, first=start > 0 and i == start)
                aux = self.x0_prev if plan.multistep else noise.draw() if plan.adds_noise(coeffs) else None
                if plan.unipc:
                    unipc_step(eps[0], x, self.unipc_history, model_in[0], guidance, coeffs, plan.input_scale(i + 1))
                elif self.windowed:
                    window_step(eps, x, aux, model_in, self.starts, self.profile, guidance, coeffs, plan.input_scale(i + 1),
                                plan.multistep)
                else:
                    if masked:                              # without a mask nothing is pinned: the plain step kernels
                        region = self.region + (plan.noise_level(i + 1),)
                    step(eps[0], x, aux, model_in[0], guidance, coeffs, plan.input_scale(i + 1), plan.multistep, region)
                noise.done()
                if callback is not None and i % callback_steps == 0:
                    callback(i, plan.timesteps[i], x)
        return x


def forward_keywords(layer_cache_mode) -> dict:
    """The keywords a loop's forward adds to its UNet call: `layer_cache` only where the cache is on, so that any UNet-shaped
    callable serves without it."""
    return {"layer_cache": layer_cache_mode} if layer_cache_mode else {}
