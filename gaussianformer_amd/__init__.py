"""MI355X-native (gfx950 / CDNA4) implementation of GaussianFormer's hot path:
the Gaussian-to-voxel splat (``LocalAggregator``) and the multi-scale deformable image
cross-attention sampler (``DeformableAggregationFunction``).  Hand-written HIP kernels
behind a C-ABI shared library (``include/gf_hip.h``); this package is the Python host side
that mirrors the reference's operator API."""
__version__ = "0.1.0"

__all__ = ["GaussianOccEncoder", "GaussianHead", "deformable_logits_autograd", "DeformLogitsFunction"]


def __getattr__(name):
    # (on first use: the package itself stays importable without torch being loaded)
    if name == "GaussianOccEncoder":
        from .encoder import GaussianOccEncoder
        return GaussianOccEncoder
    if name == "GaussianHead":
        from .head import GaussianHead
        return GaussianHead
    if name in ("deformable_logits_autograd", "DeformLogitsFunction"):
        from . import deformable_block
        return getattr(deformable_block, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
