"""The package's TTV_* environment switches are read here and nowhere else.

Every switch is an A/B or diagnostics knob; tools/README.md lists each with its default and what it selects, and
tests/test_switches_cpu.py holds that table to the reads in the code.  Nothing is cached: a call reads the environment when it
is made, so a module-level call is an import-time read and a call inside a function a call-time read.  The whole value is compared
(the C side, ttv_env_flag in csrc/ttv_common.h, looks at the first character only).
"""
from __future__ import annotations

import os


def flag(name: str, default_on: bool) -> bool:
    """A default-on switch is off only when set to "0"; a default-off switch is on only when set to "1"."""
    v = os.environ.get(name)
    return v != "0" if default_on else v == "1"


def integer(name: str, default: int) -> int:
    v = os.environ.get(name)
    return default if v is None else int(v)


def text(name: str) -> str | None:
    """The raw value, None when unset (paths, three-state switches, cache keys)."""
    return os.environ.get(name)
