"""The fused engine's ``MULTIGRAD_*`` settings (docs/api.md), read into one record."""
from __future__ import annotations

import dataclasses
from typing import Optional

from ._env import env_choice, env_flag, env_float, env_int, env_str


def _env(reader, name: str, default=None, *args):
    """A field read from ``MULTIGRAD_<name>`` when the record is made."""
    return dataclasses.field(default_factory=lambda: reader("MULTIGRAD_" + name, default, *args))


def _count(name: str, default: int) -> int:
    return max(1, env_int(name, default))


_AUTO = ("auto", "on", "off")


@dataclasses.dataclass(frozen=True)
class _Settings:
    """``_Settings()`` is the environment as it is now.  The first group counts when the
    engine is constructed (None: the keyword or the default decides); the rest is read
    again at the start of every ``setup()`` (:meth:`reread`), so a model's cached engine
    follows the environment of each run."""
    zero: Optional[bool] = _env(env_flag, "ZERO")
    owner: Optional[bool] = _env(env_flag, "OWNER")
    repartition: Optional[bool] = _env(env_flag, "REPARTITION")
    graph: Optional[bool] = _env(env_flag, "GRAPH")
    chunks: int = _env(env_int, "CHUNKS", 0)  # 0: not given
    graph_steps: int = _env(_count, "GRAPH_STEPS", 16)
    step_replay: bool = _env(env_flag, "STEP_REPLAY", False)
    device_step: bool = _env(env_flag, "DEVICE_STEP", False)
    fused_vjp_adam: bool = _env(env_flag, "FUSED_VJP_ADAM", True)
    fused_epilogue: bool = _env(env_flag, "FUSED_EPILOGUE", True)
    # ---- every setup()
    # auto (default) -- the setup autotune and the settle steps get at most
    # MULTIGRAD_TUNE_BUDGET (0.1) of the requested run's estimated time, and a run too short
    # for the minimum windows keeps the default schedule (the first candidate); on -- always
    # the full autotune (bench.py); off -- never
    autotune: str = _env(env_choice, "AUTOTUNE", "auto", _AUTO)
    autotune_window_ms: float = _env(env_float, "AUTOTUNE_WINDOW_MS", 30.0)
    autotune_rounds: int = _env(_count, "AUTOTUNE_ROUNDS", 2)
    tune_budget: float = _env(env_float, "TUNE_BUDGET", 0.1)
    settle_ms: float = _env(env_float, "SETTLE_MS", 60.0)
    max_chunks: int = _env(env_int, "MAX_CHUNKS", 4)
    side_stream: str = _env(env_choice, "TWOSHOT_SIDE_STREAM", "auto", _AUTO)  # auto: measured
    hashed_exchange: str = _env(env_choice, "HASHED_EXCHANGE", "auto", ("auto", "twoshot", "rccl"))
    twoshot_fused: str = _env(env_choice, "TWOSHOT_FUSED", "auto", _AUTO)
    twoshot_blocks: int = _env(env_int, "TWOSHOT_BLOCKS", 256)
    ag_comm: bool = _env(env_flag, "AG_COMM", True)
    pipeline: bool = _env(env_flag, "PIPELINE", True)
    fold_epilogue: bool = _env(env_flag, "FOLD_EPILOGUE", True)
    relayout: bool = _env(env_flag, "RELAYOUT", True)
    relayout_every: int = _env(env_int, "RELAYOUT_EVERY", 16)
    relayout_margin: float = _env(env_float, "RELAYOUT_MARGIN", 0.02)
    relayout_band: float = _env(env_float, "RELAYOUT_BAND", 0.02)
    err_check_every: int = _env(env_int, "ERR_CHECK_EVERY", 100)
    autotune_fault: Optional[str] = _env(env_str, "AUTOTUNE_FAULT")  # test hooks
    lbfgs_fault: Optional[str] = _env(env_str, "LBFGS_FAULT")

    def reread(self) -> "_Settings":
        """The environment now, with the construction-time group as it was read then."""
        was = dataclasses.asdict(self)
        return dataclasses.replace(_Settings(), **{
            k: was[k] for k in ("zero", "owner", "repartition", "graph", "chunks", "graph_steps",
                                "step_replay", "device_step", "fused_vjp_adam", "fused_epilogue")})
