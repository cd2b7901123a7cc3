"""``multigrad.hmc`` -> :mod:`multigrad_amd.optim.hmc` (beyond the reference, which has no
sampler)."""
from multigrad_amd.optim.hmc import (run_hmc, hmc_sample, KeyNoise, HMCResult,  # noqa: F401
                                     warmup_windows)
from multigrad_amd.utils.random import init_randkey  # noqa: F401

from multigrad_amd.utils.progress import (trange_no_tqdm, make_trange_with_tqdm,  # noqa: E402,F401
                                          make_module_trange)

trange_with_tqdm = make_trange_with_tqdm('HMC Sampling Progress')
hmc_trange = make_module_trange('HMC Sampling Progress')


def __getattr__(name):
    # the import-time MPI globals every module of the alias package has
    if name in ("COMM", "RANK", "N_RANKS"):
        import multigrad_amd
        return getattr(multigrad_amd, name)
    raise AttributeError(name)
