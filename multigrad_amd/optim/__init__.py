"""Optimizers: fixed-step GD (utils.util), Adam (fused HIP update), L-BFGS-B (host scipy)
and device L-BFGS with all-reduced dot products; the HMC sampler (``hmc``)."""
from . import adam, bfgs, hmc, prior, transforms  # noqa: F401
from .adam import Adam, run_adam, run_adam_unbounded
from .bfgs import run_bfgs

__all__ = ["adam", "bfgs", "hmc", "prior", "transforms", "Adam", "run_adam", "run_adam_unbounded", "run_bfgs",
           "run_gauss_newton_box"]


def __getattr__(name):  # lazy: the Gauss-Newton drivers import scipy.sparse
    if name == "run_gauss_newton_box":
        from .gauss_newton_box import run_gauss_newton_box
        return run_gauss_newton_box
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
