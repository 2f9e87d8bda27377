"""DPM-Solver++ multistep scheduler (data prediction, orders 1 and 2: "DPM-Solver++(2M)", Lu et al. 2022, arXiv:2211.01095)
with the surface `VideoGenPipeline` / `VideoUpscalePipeline` use.  The reference types its pipelines' `scheduler` as
`KarrasDiffusionSchedulers`, which includes diffusers' `DPMSolverMultistepScheduler`; this is the class a user brings for it.

PARITY WITH DIFFUSERS IS UNPINNED.  The class has no source in the reference tree and diffusers is not installed where this
project is tested, so nothing here is compared with diffusers' implementation.  What is pinned instead (tests/
test_dpmsolver_host.py): order 1 reproduces the reference's vendored DDIM class (eta = 0) on tests/golden/ddim_steps.pt, the
solver's accuracy on a problem with a known solution, and `coefficients` against `step`.

With alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda = log(alpha / sigma), a step from s (the current timestep) to
t (the next one), h = lambda_t - lambda_s, h_prev = the previous step's h and r = h_prev / h:

    x_t = (sigma_t / sigma_s) x_s - alpha_t (exp(-h) - 1) D,      D = x0_s + (x0_s - x0_prev) / (2 r)

`coefficients(timestep)` gives one step in the form of the fused HIP kernel (`lavie_cfg_multistep_step`):
    x0 = k_x x - k_eps m;   D = x0 + c_prev (x0 - x0_prev)  (c_prev != 0)  or  x0;   x' = c_xt x + c_x0 D
with c_xt = sigma_t / sigma_s, c_x0 = -alpha_t expm1(-h), c_prev = 1 / (2 r).  The step is first order (c_prev = 0) on the
first step, whenever solver_order == 1, on the last step when `lower_order_final` and fewer than 15 steps, and always when the
target has sigma_t = 0 (the final step to abar = 1 under `set_alpha_to_one`: h is infinite, c_xt = 0, c_x0 = 1).
Constants are computed in float64 and handed to the kernel as fp32, as the DDIM mirror does.  Order 1 is DDIM with eta = 0.

The timestep table is the DDIM mirror's ("leading" spacing, `steps_offset`, `set_alpha_to_one`), so that order 1 visits the
timesteps DDIM visits.  (`set_alpha_to_one` is this mirror's name for where the last step lands: abar = 1, what later
diffusers versions call final_sigmas_type="zero", or the first entry of the table, "sigma_min".)"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple, Union

import numpy as np
import torch


@dataclass
class DPMSolverMultistepSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


class DPMSolverMultistepScheduler:
    order = 1                  # model evaluations per step (diffusers' meaning of the attribute), not the solver order
    multistep = True           # `coefficients` returns (k_x, k_eps, c_x0, c_xt, c_prev): the pipelines keep an x0 history

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint",
                 lower_order_final: bool = True, use_karras_sigmas: bool = False, set_alpha_to_one: bool = False,
                 steps_offset: int = 1, timestep_spacing: str = "leading"):
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={algorithm_type!r} (only 'dpmsolver++' is built)")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type={solver_type!r} (only 'midpoint' is built)")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order!r} (orders 1 and 2 are built)")
        if thresholding:
            raise NotImplementedError("thresholding=True is not supported")
        if use_karras_sigmas:
            raise NotImplementedError("use_karras_sigmas=True is not supported")
        if timestep_spacing != "leading":
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r} (only 'leading' is built)")
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        if trained_betas is not None:
            betas = torch.as_tensor(np.asarray(trained_betas), dtype=torch.float32).reshape(-1)
            if betas.numel() != num_train_timesteps:
                raise ValueError(f"trained_betas has {betas.numel()} entries, num_train_timesteps is {num_train_timesteps}")
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for DPMSolverMultistepScheduler")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)
        self._index = {}
        self._x0_prev: Optional[torch.Tensor] = None
        self._next = 0                # position in `timesteps` of the step `step()` expects next
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
            use_karras_sigmas=use_karras_sigmas, set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset,
            timestep_spacing=timestep_spacing)

    _CONFIG_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order",
                    "prediction_type", "thresholding", "algorithm_type", "solver_type", "lower_order_final", "use_karras_sigmas",
                    "set_alpha_to_one", "steps_offset", "timestep_spacing")
    # Keys of a diffusers scheduler_config.json that this class does not model: key -> the values under which a diffusers
    # scheduler would do what this one does.  Any other value changes the schedule or the step and raises in from_config.
    # Keys that act only behind a flag the constructor refuses (dynamic_thresholding_ratio, sample_max_value: thresholding) or
    # that no built path reads (_class_name, _diffusers_version, clip_sample, ...) are inert and are ignored.
    _UNMODELLED_DEFAULTS = {"use_lu_lambdas": (False,), "use_exponential_sigmas": (False,), "use_beta_sigmas": (False,),
                            "use_flow_sigmas": (False,), "euler_at_final": (False,), "rescale_betas_zero_snr": (False,),
                            "lambda_min_clipped": (-math.inf,), "variance_type": (None,)}

    @classmethod
    def from_config(cls, config, **overrides):
        """Builds the scheduler from the fields of a diffusers `scheduler_config.json` (a dict, an object with attributes such
        as another scheduler's `.config`, or a path to the file); `overrides` win over the file.  `final_sigmas_type`
        ("zero" / "sigma_min") is read as `set_alpha_to_one` when that key is absent."""
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
        if "set_alpha_to_one" not in merged and "final_sigmas_type" in merged:
            kind = merged["final_sigmas_type"]
            if kind not in ("zero", "sigma_min"):
                raise NotImplementedError(f"from_config: final_sigmas_type={kind!r}")
            merged["set_alpha_to_one"] = kind == "zero"
        return cls(**{k: merged[k] for k in cls._CONFIG_KEYS if k in merged})

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def set_timesteps(self, num_inference_steps: int, device: Union[str, torch.device, None] = None):
        """The DDIM mirror's table (scheduling_ddim.py `set_timesteps`, "leading"); forgets the multistep history."""
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
        self._index = {int(t): i for i, t in enumerate(ts)}
        self._x0_prev = None
        self._next = 0

    # ------------------------------------------------------------------ constants (float64)
    def _abar(self, t: int) -> float:
        return float(self.alphas_cumprod[t].double()) if t >= 0 else float(self.final_alpha_cumprod.double())

    @staticmethod
    def _lambda(abar: float) -> float:
        return 0.5 * (math.log(abar) - math.log1p(-abar)) if abar < 1.0 else math.inf

    def _position(self, timestep) -> int:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        i = self._index.get(int(timestep))
        if i is None:
            raise ValueError(f"timestep {timestep} is not one of the {self.num_inference_steps} timesteps of this schedule")
        return i

    def noise_level(self, timestep=None) -> Tuple[float, float]:
        """(a, s) of `timestep`: a sample there is a x_0 + s noise, a = sqrt(abar_t), s = sqrt(1 - abar_t).  `None` stands for
        "after the last step": (1, 0).  What the known-region step kernels re-noise the pinned latents with."""
        if timestep is None:
            return 1.0, 0.0
        ab = float(self.alphas_cumprod[int(timestep)].double())
        return ab ** 0.5, (1.0 - ab) ** 0.5

    def coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(k_x, k_eps, c_x0, c_xt, c_prev) of the step that leaves `timestep` (module docstring).  A pure function of the
        timestep table: the position of `timestep` in it says whether there is a history and what the previous h was."""
        i = self._position(timestep)
        s = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        a_s, a_t = self._abar(s), self._abar(s - ratio)
        sa, sb = a_s ** 0.5, (1.0 - a_s) ** 0.5
        kind = self.config.prediction_type
        if kind == "epsilon":
            k_x, k_m = 1.0 / sa, sb / sa
        elif kind == "v_prediction":
            k_x, k_m = sa, sb
        else:
            k_x, k_m = 0.0, -1.0                                   # x0 = m
        sigma_t = (1.0 - a_t) ** 0.5
        if sigma_t == 0.0:                                         # h infinite: the step lands on the x0 prediction
            return k_x, k_m, 1.0, 0.0, 0.0
        lam_s = self._lambda(a_s)
        h = self._lambda(a_t) - lam_s
        c_xt = sigma_t / sb
        c_x0 = -(a_t ** 0.5) * math.expm1(-h)
        last = i == self.num_inference_steps - 1
        first_order = (self.config.solver_order == 1 or i == 0
                       or (last and self.config.lower_order_final and self.num_inference_steps < 15))
        if first_order:
            return k_x, k_m, c_x0, c_xt, 0.0
        h_prev = lam_s - self._lambda(self._abar(int(self.timesteps[i - 1])))
        return k_x, k_m, c_x0, c_xt, h / (2.0 * h_prev)            # 1 / (2 r), r = h_prev / h

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True):
        """One step in plain torch, in the dtype of `sample` (fp32 in the tests, host tensors allowed), the same update the
        fused kernel runs with `coefficients`.  Keeps its own x0 history: steps must be taken in the order of `timesteps`,
        and `set_timesteps` (or stepping from the first timestep again) starts a new trajectory."""
        i = self._position(timestep)
        if i == 0:
            self._x0_prev = None
        elif i != self._next:
            raise ValueError(f"step(): timestep {int(timestep)} is position {i} of the schedule, expected position {self._next} "
                             "(a multistep solver takes its steps in order; call set_timesteps to start again)")
        k_x, k_m, c_x0, c_xt, c_prev = self.coefficients(timestep)
        x0 = k_x * sample - k_m * model_output
        d = x0 + c_prev * (x0 - self._x0_prev) if c_prev != 0.0 else x0
        prev_sample = c_xt * sample + c_x0 * d
        self._x0_prev = x0
        self._next = i + 1
        if not return_dict:
            return (prev_sample,)
        return DPMSolverMultistepSchedulerOutput(prev_sample=prev_sample, pred_original_sample=x0)
