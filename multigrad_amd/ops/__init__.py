"""Device ops: hand-written gfx950 HIP kernels (``csrc/``) behind thin Python wrappers."""
from ._ext import available, ext

__all__ = ["available", "ext", "gaussian_binned_sum", "gaussian_binned_sum_2d",
           "gaussian_binned_sum_multi", "gaussian_binned_sum_by_group",
           "gaussian_binned_sum_fine", "FineBins", "GroupIndex", "group_gather", "segment_sum",
           "weighted_gram", "box_dual_pass"]


def __getattr__(name):  # lazy: importing the package loads no op module and no device
    if name == "gaussian_binned_sum":
        from .binned import gaussian_binned_sum
        return gaussian_binned_sum
    if name == "gaussian_binned_sum_2d":
        from .binned2d import gaussian_binned_sum_2d
        return gaussian_binned_sum_2d
    if name == "gaussian_binned_sum_multi":
        from .binned_multi import gaussian_binned_sum_multi
        return gaussian_binned_sum_multi
    if name == "gaussian_binned_sum_by_group":
        from .binned_group import gaussian_binned_sum_by_group
        return gaussian_binned_sum_by_group
    if name in ("gaussian_binned_sum_fine", "FineBins"):
        from . import binned_fine
        return getattr(binned_fine, name)
    if name in ("GroupIndex", "group_gather", "segment_sum"):
        from . import groups
        return getattr(groups, name)
    if name == "weighted_gram":
        from .gram import weighted_gram
        return weighted_gram
    if name == "box_dual_pass":
        from .box_dual import box_dual_pass
        return box_dual_pass
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
