"""pandepth_amd — MI355X-native per-base depth engine (PanDepth-compatible).

The product is the C-ABI shared library `libpandepth_amd.so` (include/pandepth_amd.h) built from
hand-written gfx950 HIP kernels, plus the C++ host side (`pandepth` CLI).  This package is only
the thin ctypes mirror of that ABI used by tests and bench.py.  It never falls back to a CPU
implementation: if the library is missing or no gfx950 device is present, it raises.
"""
from .capi import Comm, comm_unique_id, DecodeSession, Engine, PD_DECODE_COMPACT, PD_DECODE_DELETIONS, PD_DECODE_FRAGMENTS, PD_DECODE_RECORD_STATS, PD_DECODE_ROW_COUNTS, PD_DECODE_ALN_STATS, PD_ALNSTAT_WORDS, PD_RECSTAT_FIXED, PD_ROWCOUNT_WORDS, PD_UNIT_GUESS, PdError, lib_path, load, PD_PUSH_SORTED, PD_PUSH_DEFAULT, PD_PUSH_DISORDER, PD_PUSH_MORE  # noqa: F401

__version__ = "0.1.0"
