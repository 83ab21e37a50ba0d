"""MI355X-native TiTok-Video tokenizer hot path (encode -> FSQ -> decode).

Host side is Python on PyTorch-ROCm (device memory, streams, torch.distributed); the compute path is
hand-written HIP for gfx950 behind the C-ABI in include/titok_hip.h (libtitok_hip.so, loaded lazily by
`titok_video_amd._lib`).  There is no CPU or eager-PyTorch fallback: ops raise if the library is missing.
"""
__version__ = "0.1.0"


def set_deterministic(flag: bool) -> bool:
    """Deterministic training: with the mode on, every gradient sum of the HIP path has a fixed order (two runs on the same inputs give
    the same bits); off (the default) the faster atomics.  Process-wide; returns the previous setting.  `TTV_DETERMINISTIC=1` starts a
    process with the mode on.  The order of a cross-rank all-reduce is not covered."""
    from . import _lib
    return _lib.set_deterministic(flag)


def is_deterministic() -> bool:
    from . import _lib
    return _lib.is_deterministic()
