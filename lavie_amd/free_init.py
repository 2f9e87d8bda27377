"""FreeInit (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models", ECCV 2024; diffusers' FreeInitMixin): the
setting, its low-pass filter, and the state one sampling call keeps between its iterations.  DESIGN.md 7.15.

A call with FreeInit samples `num_iters` times.  Between two iterations the result x0 is re-noised to the last training timestep,
z_T = a x0 + s e0 (e0: the unit noise the call started from), and its spatio-temporal low band is joined with the high band of fresh
noise z scaled by r = init_noise_sigma:

    mixed = r z + Re IFFT3( LPF .* FFT3(z_T - r z) )           over (F, H, W), per (video, channel)

which one launch sequence of `ops.freq_mix` (csrc/freq_mix.hip) computes, writing the next iteration's fp32 latents and fp16 model
input.  The filter is built here, on the CPU in fp64: the published filter over the fftshift-ed spectrum, its EVEN part
(LPF(k) + LPF(-k)) / 2 (for an odd axis length the published filter is not even and `.real` of the published result keeps exactly
this part), un-shifted to FFT-native order, rounded to fp32."""
import math

import torch

METHODS = ("butterworth", "gaussian", "ideal")


def freq_filter(F: int, H: int, W: int, method: str = "butterworth", order: int = 4, spatial_stop_frequency: float = 0.25,
                temporal_stop_frequency: float = 0.25) -> torch.Tensor:
    """The even part of FreeInit's low-pass filter for an [F, H, W] volume, fp32 [F, H, W] on the CPU in FFT-native order
    (frequency 0 at index 0).  Over the shifted spectrum the published filter is a function of
    d^2 = ((ds / dt) (2 t / F - 1))^2 + (2 h / H - 1)^2 + (2 w / W - 1)^2, ds / dt the spatial / temporal stop frequency:
    butterworth 1 / (1 + (d^2 / ds^2)^order), gaussian exp(-d^2 / (2 ds^2)), ideal [d^2 <= (2 ds)^2]; all zeros when ds or dt is 0."""
    if method not in METHODS:
        raise ValueError(f"`method` must be one of {METHODS} but is {method!r}")
    if min(F, H, W) < 1:
        raise ValueError(f"the filter's shape must be positive, got {(F, H, W)}")
    ds, dt = float(spatial_stop_frequency), float(temporal_stop_frequency)
    if ds == 0.0 or dt == 0.0:
        return torch.zeros((F, H, W), dtype=torch.float32)
    axis = [2.0 * torch.arange(n, dtype=torch.float64) / n - 1.0 for n in (F, H, W)]
    d2 = ((ds / dt) * axis[0])[:, None, None] ** 2 + axis[1][None, :, None] ** 2 + axis[2][None, None, :] ** 2
    if method == "butterworth":
        lpf = 1.0 / (1.0 + (d2 / ds ** 2) ** int(order))
    elif method == "gaussian":
        lpf = torch.exp(-d2 / (2.0 * ds ** 2))
    else:
        lpf = (d2 <= (2.0 * ds) ** 2).to(torch.float64)
    # index n of the shifted spectrum holds frequency n - N // 2: rolling by -(N // 2) puts frequency 0 first (ifftshift)
    native = torch.roll(lpf, shifts=[-(n // 2) for n in (F, H, W)], dims=(0, 1, 2))
    # frequency -k lives at index (-k) mod N: reverse every axis, then bring index 0 back to the front
    mirrored = torch.roll(torch.flip(native, dims=(0, 1, 2)), shifts=(1, 1, 1), dims=(0, 1, 2))
    return ((native + mirrored) / 2.0).to(torch.float32)


class FreeInit:
    """The setting, with diffusers' names and defaults (FreeInitMixin.enable_free_init)."""

    def __init__(self, num_iters: int = 3, use_fast_sampling: bool = False, method: str = "butterworth", order: int = 4,
                 spatial_stop_frequency: float = 0.25, temporal_stop_frequency: float = 0.25):
        if isinstance(num_iters, bool) or not isinstance(num_iters, int) or num_iters < 1:
            raise ValueError(f"`num_iters` must be an integer >= 1 but is {num_iters!r}")
        if method not in METHODS:
            raise ValueError(f"`method` must be one of {METHODS} but is {method!r}")
        if isinstance(order, bool) or not isinstance(order, int) or order < 1:
            raise ValueError(f"`order` must be an integer >= 1 but is {order!r}")
        for name, v in (("spatial_stop_frequency", spatial_stop_frequency), ("temporal_stop_frequency", temporal_stop_frequency)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"`{name}` must be a finite number >= 0 but is {v!r}")
        self.num_iters, self.use_fast_sampling, self.method, self.order = num_iters, bool(use_fast_sampling), method, order
        self.spatial_stop_frequency, self.temporal_stop_frequency = float(spatial_stop_frequency), float(temporal_stop_frequency)

    def steps_at(self, i: int, num_inference_steps: int) -> int:
        """Denoising steps of iteration i: with `use_fast_sampling` max(1, int(n / num_iters (i + 1))) (diffusers' coarse-to-fine
        schedule; the last iteration takes all n), otherwise n every time."""
        if not 0 <= i < self.num_iters:
            raise ValueError(f"iteration {i} outside 0..{self.num_iters - 1}")
        if not self.use_fast_sampling:
            return int(num_inference_steps)
        return max(1, int(num_inference_steps / self.num_iters * (i + 1)))

    def filter(self, F: int, H: int, W: int) -> torch.Tensor:
        return freq_filter(F, H, W, self.method, self.order, self.spatial_stop_frequency, self.temporal_stop_frequency)

    def __repr__(self):
        return (f"FreeInit(num_iters={self.num_iters}, use_fast_sampling={self.use_fast_sampling}, method={self.method!r}, "
                f"order={self.order}, spatial_stop_frequency={self.spatial_stop_frequency}, "
                f"temporal_stop_frequency={self.temporal_stop_frequency})")


def coerce(setting):
    """None, a FreeInit or a mapping of its keywords -> None (off: absent or num_iters == 1, the call without it) or a FreeInit."""
    if setting is None:
        return None
    if not isinstance(setting, FreeInit):
        setting = FreeInit(**dict(setting))
    return setting if setting.num_iters > 1 else None


class FreeInitRun:
    """What one sampling call keeps for its iterations, allocated once in front of the loop: the call's initial latents (= r e0, on
    the device), the filter on the device, the buffer of the fresh noise and the transform workspace.  `remix` enqueues the mix
    between two iterations: it draws z from `generator` as `randn_tensor` draws initial latents, and `ops.freq_mix` overwrites x
    with the next iteration's latents and, where given, fills the next fp16 model input in the same launch."""

    def __init__(self, setting: FreeInit, scheduler, x: torch.Tensor, generator=None, plan_at=None):
        from . import ops
        self.setting, self.generator, self._scheduler = setting, generator, scheduler
        self.plan_at = plan_at                                           # iteration -> its step plan (the loop's own kind)
        self.start = x.clone()                                           # r e0
        self.filter = setting.filter(*x.shape[2:]).to(x.device)
        images = x.shape[0] * x.shape[1]
        need = ops.freq_mix_workspace_bytes(images, *x.shape[2:])
        if need == 0:
            raise ValueError(f"FreeInit: latents {tuple(x.shape)} are outside the frequency mix's range (F <= 256, H, W <= 128)")
        self.workspace = torch.empty(need // 4, dtype=torch.float32, device=x.device)

    def remix(self, x: torch.Tensor, model_in, input_scale: float):
        from . import ops
        from .scheduling_ddpm import randn_tensor
        r = float(self._scheduler.init_noise_sigma)
        a, s = self._scheduler.noise_level(self._scheduler.config.num_train_timesteps - 1)
        z = randn_tensor(tuple(x.shape), generator=self.generator, device=x.device, dtype=torch.float32)
        # `start` holds r e0, so s e0 = (s / r) start: one rounding in a scalar instead of a division per element
        ops.freq_mix(x, self.start, z, self.filter, a, s / r, r, out=x, model_in=model_in, input_scale=input_scale,
                     workspace=self.workspace)
