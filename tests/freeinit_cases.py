"""Shapes and seeded inputs of the FreeInit tests (tests/test_freeinit_host.py, tests/test_gpu_freeinit.py)."""
import torch

METHODS = ("butterworth", "gaussian", "ideal")
# (images, F, H, W): the base shape; tiny with an odd F and an odd image count; an odd prime F (the even part matters); a unit axis
# with odd spatial sizes; just past a power of two; both maxima
SHAPES = [(4, 16, 40, 64), (3, 5, 6, 8), (2, 61, 10, 12), (1, 1, 7, 9), (2, 8, 65, 33), (1, 256, 4, 128)]
ALL_METHOD_SHAPES = SHAPES[:3]
OP_CASES = [(shape, m) for shape in ALL_METHOD_SHAPES for m in METHODS] + [(shape, "butterworth") for shape in SHAPES[3:]]
ORDER, DS, DT = 4, 0.25, 0.25
R_VALUES = (1.0, 1.7)                # init_noise_sigma of DDPM / DDIM / DPM-Solver++, and a non-unit value
IN_SCALE = 0.8125                    # a model-input scale != 1
# filter shapes of the host test: odd lengths, unit axes, and stop frequencies that differ
FILTER_SHAPES = [(16, 40, 64), (5, 6, 8), (61, 10, 12), (1, 7, 9), (3, 1, 1), (7, 5, 3)]
FILTER_STOPS = [(0.25, 0.25), (0.5, 0.125), (0.3, 1.0), (0.0, 0.25), (0.25, 0.0)]


def noise_level():
    """(a, s) of the last training timestep under the DDPM scheduler's defaults."""
    from lavie_amd.scheduling_ddpm import DDPMScheduler
    sch = DDPMScheduler()
    return sch.noise_level(sch.config.num_train_timesteps - 1)


def op_inputs(shape, seed=0):
    """x0, e0, z: N(0, 1), fp32 [images, F, H, W]."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * sum(shape))
    return tuple(torch.randn(shape, generator=g, dtype=torch.float32) for _ in range(3))
