"""UniPC multistep scheduler (Zhao et al., "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models",
arXiv:2302.04867; diffusers' `UniPCMultistepScheduler`) with the surface `VideoGenPipeline` / `VideoUpscalePipeline` use: data
prediction, B(h) = e^h - 1 ("bh2"), orders 1 and 2, the last step onto sigma = 0.

PARITY WITH DIFFUSERS IS UNPINNED.  diffusers is not installed where this project is tested, so nothing here is compared with its
implementation.  What is pinned instead (tests/test_unipc_host.py): `coefficients` and `step` against an independent float64
restatement of the paper's update (tests/unipc_reference.py), and the solver's accuracy on a Gaussian problem whose probability-flow
ODE has a closed form, against this package's DPM-Solver++ 2M and against UniPC without its corrector.

With alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda = log(alpha / sigma), positions i = 0 .. N-1 of the timestep
table (position N is sigma = 0), x_i the predicted sample the model is evaluated at, m_i its x0 prediction, h_i = lambda_i -
lambda_{i-1} and A(h) = -alpha expm1(-h) = alpha (1 - e^{-h}):

  corrector (UniC; i >= 1; order q = the order of the predictor that produced x_i), from the previous CORRECTED sample:
      x_i^c = (sigma_i / sigma_{i-1}) x_{i-1}^c + A_i m_{i-1} + A_i [ rho_1 (m_{i-2} - m_{i-1}) / r + rho_q (m_i - m_{i-1}) ]
      q = 1: rho_1 = 1/2, no m_{i-2} term.  q = 2: r = (lambda_{i-2} - lambda_{i-1}) / h_i and (rho_1, rho_2) solve
      [[1, 1], [r, 1]] rho = (b_1, b_2), b_k = k! phi_{k+1}(-h) / B(-h) in diffusers' notation, in float64 on the host.
  predictor (UniP; order p = 1 at position 0 and at position N-1, whose target has sigma = 0, with `lower_order_final` and
  without it (`predictor_order`); else `solver_order`), from x_i^c:
      x_{i+1} = (sigma_{i+1} / sigma_i) x_i^c + A_{i+1} m_i + A_{i+1} (1/2) (m_{i-1} - m_i) / r',  r' = -h_i / h_{i+1}   (p = 2)
  The model output x_i^c's step needs is the one the predictor needs anyway: the corrector costs no model evaluation.

`coefficients(timestep)` gives the step that leaves `timestep` in the form of the fused HIP kernel (`lavie_cfg_unipc_step`):
    m = k_x x - k_eps eps;   xc = corr ? c_l x_last + c_0 m + c_1 m1 + c_2 m2 : x;   x' = p_x xc + p_0 m + p_1 m1
    x_last <- xc, m2 <- m1, m1 <- m        (x_last = x_{i-1}^c, m1 = m_{i-1}, m2 = m_{i-2})
v-prediction is folded into (k_x, k_eps) as in the DPM-Solver++ mirror.  Constants are derived in float64 and handed to the kernel
as fp32.  The last step has sigma = 0: h is infinite, (p_x, p_0, p_1) = (0, 1, 0) and the step returns the x0 prediction.

The timestep table is the DDIM mirror's ("leading" spacing, `steps_offset`), as in the DPM-Solver++ mirror."""
import math
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple, Union

import numpy as np
import torch


@dataclass
class UniPCMultistepSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


# one step in the fused kernel's form (module docstring); corr is a bool, the rest floats
UniPCCoefficients = namedtuple("UniPCCoefficients", "k_x k_eps corr c_l c_0 c_1 c_2 p_x p_0 p_1")


class UniPCMultistepScheduler:
    order = 1                  # model evaluations per step (diffusers' meaning of the attribute), not the solver order
    unipc = True               # `coefficients` returns UniPCCoefficients: the pipelines keep x_last, m1, m2 beside the latents

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, predict_x0: bool = True, solver_type: str = "bh2", lower_order_final: bool = True,
                 disable_corrector=(), use_karras_sigmas: bool = False, timestep_spacing: str = "leading", steps_offset: int = 1,
                 final_sigmas_type: str = "zero"):
        if solver_type != "bh2":
            raise NotImplementedError(f"solver_type={solver_type!r} (only 'bh2' is built)")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order!r} (orders 1 and 2 are built)")
        if not predict_x0:
            raise NotImplementedError("predict_x0=False (the noise-prediction form) is not supported")
        if thresholding:
            raise NotImplementedError("thresholding=True is not supported")
        if use_karras_sigmas:
            raise NotImplementedError("use_karras_sigmas=True is not supported")
        if timestep_spacing != "leading":
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r} (only 'leading' is built)")
        if final_sigmas_type != "zero":
            raise NotImplementedError(f"final_sigmas_type={final_sigmas_type!r} (only 'zero' is built: the last step lands on sigma = 0)")
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        disable_corrector = [int(i) for i in disable_corrector]
        if trained_betas is not None:
            betas = torch.as_tensor(np.asarray(trained_betas), dtype=torch.float32).reshape(-1)
            if betas.numel() != num_train_timesteps:
                raise ValueError(f"trained_betas has {betas.numel()} entries, num_train_timesteps is {num_train_timesteps}")
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for UniPCMultistepScheduler")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)
        self._index = {}
        self._history = None          # (x_last, m1, m2) of `step()`
        self._next = 0                # position in `timesteps` of the step `step()` expects next
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            predict_x0=predict_x0, solver_type=solver_type, lower_order_final=lower_order_final, disable_corrector=disable_corrector,
            use_karras_sigmas=use_karras_sigmas, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
            final_sigmas_type=final_sigmas_type)

    _CONFIG_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order",
                    "prediction_type", "thresholding", "predict_x0", "solver_type", "lower_order_final", "disable_corrector",
                    "use_karras_sigmas", "timestep_spacing", "steps_offset", "final_sigmas_type")
    # Keys of a diffusers scheduler_config.json that this class does not model: key -> the values under which a diffusers
    # scheduler would do what this one does.  Any other value changes the schedule or the step and raises in from_config.
    # Keys that act only behind a flag the constructor refuses (dynamic_thresholding_ratio, sample_max_value: thresholding) or
    # that no built path reads (_class_name, _diffusers_version, solver_p, ...) are inert and are ignored.
    _UNMODELLED_DEFAULTS = {"use_exponential_sigmas": (False,), "use_beta_sigmas": (False,), "use_flow_sigmas": (False,),
                            "rescale_betas_zero_snr": (False,), "solver_p": (None,)}

    @classmethod
    def from_config(cls, config, **overrides):
        """Builds the scheduler from the fields of a diffusers `scheduler_config.json` (a dict, an object with attributes such
        as another scheduler's `.config`, or a path to the file); `overrides` win over the file."""
        if isinstance(config, (str, bytes)) or hasattr(config, "__fspath__"):
            import json
            with open(config) as fh:
                config = json.load(fh)
        elif not isinstance(config, dict):
            config = dict(vars(config))
        unknown = set(overrides) - set(cls._CONFIG_KEYS)
        if unknown:
            raise TypeError(f"from_config: unknown scheduler fields {sorted(unknown)}")
        merged = dict(config)
        merged.update(overrides)
        for key, same in cls._UNMODELLED_DEFAULTS.items():
            if key in merged and not any(merged[key] is v or merged[key] == v for v in same):
                raise NotImplementedError(f"from_config: {key}={merged[key]!r} changes the schedule / step and is not modelled "
                                          f"here (accepted: {list(same)})")
        return cls(**{k: merged[k] for k in cls._CONFIG_KEYS if k in merged})

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None):
        """The DDIM mirror's table (scheduling_ddim.py `set_timesteps`, "leading"); forgets the history of `step()`."""
        n_train = self.config.num_train_timesteps
        if not 1 <= num_inference_steps <= n_train:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} must lie in 1..{n_train} (`num_train_timesteps`)")
        self.num_inference_steps = num_inference_steps
        step_ratio = n_train // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        if ts[0] >= n_train:
            raise ValueError(f"first timestep {ts[0]} is outside the {n_train}-entry alpha table (steps_offset too large)")
        steps = torch.from_numpy(ts)
        self.timesteps = steps.to(device) if device is not None else steps
        self._table = [int(t) for t in ts]
        self._index = {int(t): i for i, t in enumerate(ts)}
        self._history = None
        self._next = 0

    # ------------------------------------------------------------------ constants (float64)
    def _level(self, position: int) -> Tuple[float, float, float]:
        """(alpha, sigma, lambda) of a position of the table; position N is the end of the run: (1, 0, inf)."""
        if position >= self.num_inference_steps:
            return 1.0, 0.0, math.inf
        ab = float(self.alphas_cumprod[self._table[position]].double())
        return ab ** 0.5, (1.0 - ab) ** 0.5, 0.5 * (math.log(ab) - math.log1p(-ab))

    def _position(self, timestep) -> int:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        i = self._index.get(int(timestep))
        if i is None:
            raise ValueError(f"timestep {timestep} is not one of the {self.num_inference_steps} timesteps of this schedule")
        return i

    def noise_level(self, timestep=None) -> Tuple[float, float]:
        """(a, s) of `timestep`: a sample there is a x_0 + s noise, a = sqrt(abar_t), s = sqrt(1 - abar_t).  `None` stands for
        "after the last step": (1, 0)."""
        if timestep is None:
            return 1.0, 0.0
        ab = float(self.alphas_cumprod[int(timestep)].double())
        return ab ** 0.5, (1.0 - ab) ** 0.5

    def predictor_order(self, position: int) -> int:
        """Order of the predictor that leaves `position`: 1 at position 0 (no history) and at the last position, else
        `solver_order`.  The last step is first order with `lower_order_final` and without it: its target has sigma = 0, where the
        second-order term of the published update is 0 / 0 (r' = -h_i / inf), so `lower_order_final` is inert here."""
        return min(self.config.solver_order, position + 1, self.num_inference_steps - position)

    def corrects(self, position: int) -> bool:
        """Whether the step at `position` runs the corrector: never at position 0; `disable_corrector` lists, as in diffusers, the
        positions whose PREDICTION is left uncorrected (position - 1 here)."""
        return position > 0 and (position - 1) not in self.config.disable_corrector

    def coefficients(self, timestep) -> UniPCCoefficients:
        """The step that leaves `timestep` in the fused kernel's form (module docstring).  A pure function of the timestep
        table: the position of `timestep` in it says which history exists and what the previous step sizes were."""
        i = self._position(timestep)
        a_i, s_i, lam_i = self._level(i)
        kind = self.config.prediction_type
        if kind == "epsilon":
            k_x, k_m = 1.0 / a_i, s_i / a_i
        elif kind == "v_prediction":
            k_x, k_m = a_i, s_i
        else:
            k_x, k_m = 0.0, -1.0                                   # x0 = m
        # ---- corrector: x_i^c from x_{i-1}^c, m1 = m_{i-1}, m2 = m_{i-2} and the fresh m = m_i
        corr, c_l, c_0, c_1, c_2 = self.corrects(i), 0.0, 0.0, 0.0, 0.0
        if corr:
            _, s_p, lam_p = self._level(i - 1)
            h = lam_i - lam_p
            big_a = -a_i * math.expm1(-h)
            c_l = s_i / s_p
            if self.predictor_order(i - 1) == 1:
                c_0, c_1 = 0.5 * big_a, 0.5 * big_a
            else:
                r = (self._level(i - 2)[2] - lam_p) / h
                # b_k = k! I_k / (h^k I_0) with I_0 = 1 - e^{-h}, I_k = h^k / k! - I_{k-1}, written as diffusers writes them
                hh = -h
                phi = math.expm1(hh) / hh - 1.0
                b_1 = phi / math.expm1(hh)
                b_2 = (phi / hh - 0.5) * 2.0 / math.expm1(hh)
                rho_1, rho_2 = np.linalg.solve(np.array([[1.0, 1.0], [r, 1.0]]), np.array([b_1, b_2]))
                c_0, c_2 = big_a * rho_2, big_a * rho_1 / r
                c_1 = big_a * (1.0 - rho_1 / r - rho_2)
        # ---- predictor: x_{i+1} from x_i^c, m = m_i and m1 = m_{i-1}
        a_n, s_n, lam_n = self._level(i + 1)
        if s_n == 0.0:                                             # h infinite: the step lands on the x0 prediction
            p_x, p_0, p_1 = 0.0, 1.0, 0.0
        else:
            h = lam_n - lam_i
            big_a = -a_n * math.expm1(-h)
            p_x, p_0, p_1 = s_n / s_i, big_a, 0.0
            if self.predictor_order(i) == 2:
                r = (self._level(i - 1)[2] - lam_i) / h
                p_0, p_1 = big_a * (1.0 - 0.5 / r), big_a * 0.5 / r
        return UniPCCoefficients(k_x, k_m, corr, float(c_l), float(c_0), float(c_1), float(c_2), p_x, p_0, p_1)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True):
        """One step in plain torch, in the dtype of `sample` (fp32 in the tests, host tensors allowed), the same update the
        fused kernel runs with `coefficients`.  Keeps its own history (x_last, m1, m2): steps must be taken in the order of
        `timesteps`, and `set_timesteps` (or stepping from the first timestep again) starts a new trajectory."""
        i = self._position(timestep)
        if i == 0:
            self._history = None
        elif i != self._next:
            raise ValueError(f"step(): timestep {int(timestep)} is position {i} of the schedule, expected position {self._next} "
                             "(a multistep solver takes its steps in order; call set_timesteps to start again)")
        c = self.coefficients(timestep)
        x_last, m1, m2 = self._history if self._history is not None else (None, None, None)
        m = c.k_x * sample - c.k_eps * model_output
        xc = sample
        if c.corr:
            xc = c.c_l * x_last + c.c_0 * m
            if c.c_1 != 0.0:
                xc = xc + c.c_1 * m1
            if c.c_2 != 0.0:
                xc = xc + c.c_2 * m2
        prev_sample = c.p_x * xc + c.p_0 * m
        if c.p_1 != 0.0:
            prev_sample = prev_sample + c.p_1 * m1
        self._history = (xc, m, m1)
        self._next = i + 1
        if not return_dict:
            return (prev_sample,)
        return UniPCMultistepSchedulerOutput(prev_sample=prev_sample, pred_original_sample=m)
