"""The denoising objective evaluated forward: what the fine-tuning loop of the reference computes per batch
(base/pipelines/fine_tuning.py:486-592) without its backward pass -- noise the clean latents at one timestep per clip, run the UNet
under the context, score the prediction against the noise (or the velocity) by a mean squared error per clip, optionally weighted by
min-SNR-gamma and with offset noise.  The two ends around the forward are one launch each (`ops.noisy_latents`, `ops.denoising_loss`)
with the noise made in registers from a `PhiloxGenerator`'s (seed, draw): no noise tensor exists, and a clip's loss has the same bits
in any batch of the operators.  Not claimed: equality with torch's or diffusers' random stream, per-frame losses, gradients."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .noise import PhiloxGenerator

PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")


def _abar(scheduler, timesteps) -> np.ndarray:
    t = [int(v) for v in (timesteps.reshape(-1).tolist() if isinstance(timesteps, torch.Tensor) else timesteps)]
    n = int(scheduler.alphas_cumprod.shape[0])
    if any(v < 0 or v >= n for v in t):
        raise ValueError(f"timesteps {t} must lie in 0..{n - 1}")
    return scheduler.alphas_cumprod.detach().cpu().to(torch.float64).numpy()[t]


def noise_levels(scheduler, timesteps) -> list:
    """[(a, s)] per timestep: a = sqrt(abar_t), s = sqrt(1 - abar_t), in float64 from `scheduler.alphas_cumprod`, each rounded once to
    fp32: the values the kernels take."""
    ab = _abar(scheduler, timesteps)
    return [(float(np.float32(np.sqrt(v))), float(np.float32(np.sqrt(1.0 - v)))) for v in ab]


def snr(scheduler, timesteps) -> torch.Tensor:
    """(a / s)^2 = abar_t / (1 - abar_t) per timestep, float64 (the reference's compute_snr)."""
    ab = _abar(scheduler, timesteps)
    return torch.from_numpy((np.sqrt(ab) / np.sqrt(1.0 - ab)) ** 2)


def min_snr_weights(snr, gamma: float, kind: str) -> torch.Tensor:
    """min(snr, gamma) / snr for "epsilon", min(snr, gamma) / (snr + 1) for "v_prediction" (Hang et al., "Efficient Diffusion
    Training via Min-SNR Weighting Strategy", sections 3.4 and 4.2; fine_tuning.py:581-588), float64."""
    snr = torch.as_tensor(snr, dtype=torch.float64)
    clipped = torch.minimum(snr, torch.full_like(snr, float(gamma)))
    if kind == "epsilon":
        return clipped / snr
    if kind == "v_prediction":
        return clipped / (snr + 1.0)
    raise ValueError(f"min-SNR weights are defined for epsilon and v_prediction, not {kind!r}")


@dataclass
class DenoisingLossOutput:
    mse: torch.Tensor          # fp32 [P]: the mean squared error of each latent, as the kernel wrote it
    weights: torch.Tensor      # float64 [P] on the host: the min-SNR weights (ones without snr_gamma)
    loss: float                # the float64 mean of mse * weights, computed on the host
    timesteps: list


class DenoisingLoss:
    """unet: the engine UNet (anything called as unet(sample, timestep, encoder_hidden_states=...).sample); scheduler: anything with
    `alphas_cumprod` and `config.prediction_type`.  `forward`: an optional callable (model_in, timesteps, encoder_hidden_states) -> pred
    in place of the plain UNet call, for models whose extra inputs the caller assembles (nothing is claimed for those here)."""

    def __init__(self, unet, scheduler, snr_gamma=None, noise_offset: float = 0.0, prediction_type=None, forward=None):
        kind = prediction_type if prediction_type is not None else scheduler.config.prediction_type
        if kind not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type {kind!r} is not one of {PREDICTION_TYPES}")
        if snr_gamma is not None and (kind == "sample" or not float(snr_gamma) > 0.0):
            raise ValueError(f"snr_gamma={snr_gamma} needs a positive value and an epsilon or v_prediction target")
        if unet is None and forward is None:
            raise ValueError("DenoisingLoss needs a unet or a forward callable")
        self.unet, self.scheduler, self.kind = unet, scheduler, kind
        self.snr_gamma = None if snr_gamma is None else float(snr_gamma)
        self.noise_offset = float(noise_offset)
        self.forward = forward if forward is not None else self._unet_forward

    def _unet_forward(self, model_in, timesteps, encoder_hidden_states):
        return self.unet(model_in, timesteps, encoder_hidden_states=encoder_hidden_states).sample

    def _timesteps(self, timesteps, latents: int) -> list:
        if isinstance(timesteps, torch.Tensor):
            timesteps = timesteps.reshape(-1).tolist()
        t = [int(timesteps)] * latents if isinstance(timesteps, (int, float)) else [int(v) for v in timesteps]
        if len(t) != latents:
            raise ValueError(f"got {len(t)} timesteps for {latents} latents")
        return t

    @torch.no_grad()
    def evaluate(self, latents, encoder_hidden_states, timesteps, generator) -> DenoisingLossOutput:
        """latents [P, C, F, h, w] fp32 or fp16, already scaled by the VAE factor; encoder_hidden_states [P, n, d] (or [1, n, d] for all);
        timesteps: one int, or one per latent; generator: a PhiloxGenerator, which this call advances by one draw (two with offset
        noise).  More than NOISE_MAX_SEEDS latents run as chunks, chunk [i, j) under the seeds of generator[i:j]."""
        if not isinstance(generator, PhiloxGenerator):
            raise TypeError(f"evaluate needs a PhiloxGenerator, got {type(generator).__name__}: the target is regenerated from (seed, "
                            "draw) inside the loss kernel, which a torch.Generator cannot give")
        if latents.dim() != 5:
            raise ValueError(f"latents must be [P, C, F, h, w], got {tuple(latents.shape)}")
        p = latents.shape[0]
        t = self._timesteps(timesteps, p)
        ctx = encoder_hidden_states
        if ctx.shape[0] not in (1, p):
            raise ValueError(f"got {ctx.shape[0]} contexts for {p} latents (expected 1 or one per latent)")
        if generator.per_latent:
            generator.seeds(p)                                   # a list of another length is refused before anything runs
        levels = noise_levels(self.scheduler, t)
        draw = generator.next_draw()
        offset_draw = generator.next_draw() if self.noise_offset != 0.0 else None
        hw = latents.shape[3] * latents.shape[4]
        latents = latents.contiguous()
        mse = torch.empty(p, dtype=torch.float32, device=latents.device)
        for i in range(0, p, _lib.NOISE_MAX_SEEDS):
            j = min(p, i + _lib.NOISE_MAX_SEEDS)
            seeds = generator[i:j].seeds(j - i)
            offset = None if offset_draw is None else (self.noise_offset, offset_draw, hw)
            x0 = latents[i:j]
            model_in = ops.noisy_latents(x0, seeds, draw, levels[i:j], offset=offset)
            t_dev = torch.tensor(t[i:j], dtype=torch.float32, device=latents.device)
            pred = self.forward(model_in, t_dev, ctx[i:j] if ctx.shape[0] == p else ctx.expand(j - i, -1, -1))
            if pred.dtype != torch.float16:
                pred = pred.to(torch.float16)
            ops.denoising_loss(pred.contiguous(), x0, seeds, draw, levels[i:j], self.kind, offset=offset, out=mse[i:j])
        if self.snr_gamma is None:
            weights = torch.ones(p, dtype=torch.float64)
        else:
            weights = min_snr_weights(snr(self.scheduler, t), self.snr_gamma, self.kind)
        loss = float((mse.detach().cpu().to(torch.float64) * weights).mean())
        return DenoisingLossOutput(mse=mse, weights=weights, loss=loss, timesteps=t)

    @torch.no_grad()
    def sweep(self, latents, encoder_hidden_states, timesteps=(999, 750, 500, 250, 0), draws: int = 1, generator=None) -> torch.Tensor:
        """The per-timestep curve: float64 [P, T] on the host, column k = the mean over `draws` draws of `evaluate(..., timesteps[k])`'s
        mse.  The columns are evaluated in order (timestep-major, then draw) on one generator (PhiloxGenerator(0) when None), so every
        (timestep, draw) has a draw number of its own."""
        draws = int(draws)
        if draws < 1:
            raise ValueError(f"draws={draws} must be >= 1")
        generator = PhiloxGenerator(0) if generator is None else generator
        cols = []
        for t in timesteps:
            runs = [self.evaluate(latents, encoder_hidden_states, int(t), generator).mse.detach().cpu().to(torch.float64)
                    for _ in range(draws)]
            cols.append(runs[0] if draws == 1 else torch.stack(runs).mean(0))
        return torch.stack(cols, dim=1)
