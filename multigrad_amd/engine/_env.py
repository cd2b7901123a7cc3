"""The one parser of the engines' ``MULTIGRAD_*`` settings.

Off is ``0/false/off/no`` and on is ``1/true/on/yes`` (any case, surrounding blanks
ignored).  An unset or empty variable, and a word the reader does not know, give the default."""
from __future__ import annotations

import os

_OFF = ("0", "false", "off", "no")
_ON = ("1", "true", "on", "yes")


def _word(name: str) -> str:
    return os.environ.get(name, "").strip().lower()


def env_flag(name: str, default=None):
    """True / False, or ``default`` (which may be None: "not decided here")."""
    w = _word(name)
    return True if w in _ON else False if w in _OFF else default


def env_int(name: str, default: int) -> int:
    w = _word(name)
    return int(w) if w else default


def env_float(name: str, default: float) -> float:
    w = _word(name)
    return float(w) if w else default


def env_str(name: str, default=None):
    """The value as it is."""
    return os.environ.get(name) or default


def env_choice(name: str, default: str, choices) -> str:
    """One of ``choices``; the on / off words count as ``"on"`` / ``"off"`` where those are
    choices."""
    w = _word(name)
    w = "on" if w in _ON else "off" if w in _OFF else w
    return w if w in choices else default
