"""lavie_amd — MI355X-native LaVie base T2V denoising path.

Hand-written gfx950 HIP kernels behind a C-ABI library (`lavie_amd/csrc`, `include/lavie_hip.h`)
plus the host-side mirror of the reference's `UNet3DConditionModel.forward` /
`VideoGenPipeline` / DDPM-scheduler surface.  There is no CPU fallback: importing the compute
entry points without the built library raises.

The encoders that feed the UNet its context run on the engine as well: `lavie_amd.text_encoder.HipCLIPTextModel`,
`lavie_amd.image_encoder.HipCLIPVisionModel` and `HipMappingNetwork` (imported on use: they need the built library).
`lavie_amd.HipCLIPImageProcessor` and `lavie_amd.ClipScorer` (lavie_amd.clip_score) turn uint8 pixels and token ids into
pixel_values, CLIP features and CLIPSIM scores; they too are imported on first use.  `lavie_amd.HipR3D18`, `VideoProcessor`,
`FvdScorer`, `FrechetStats` and `frechet_distance` (lavie_amd.fvd) score clip quality by FVD on R3D-18 features.
`lavie_amd.DenoisingLoss`, `snr` and `min_snr_weights` (lavie_amd.denoising_loss) evaluate the training objective forward: the
denoising loss of held-out clips per timestep, with the noise made in registers from a `PhiloxGenerator`.
"""
from .config import UNetConfig, BASE_CONFIG  # noqa: F401

__version__ = "0.1.0"

_LAZY = {"HipCLIPImageProcessor": "clip_score", "ClipScorer": "clip_score", "HipR3D18": "fvd", "VideoProcessor": "fvd", "FvdScorer": "fvd",
         "FrechetStats": "fvd", "frechet_distance": "fvd", "DenoisingLoss": "denoising_loss", "snr": "denoising_loss",
         "min_snr_weights": "denoising_loss"}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
