"""Device-resident matching: both full-resolution images stay in HBM, every tile of
`KLT.match` and the ZNCC scoring run on them without further host<->device image traffic.

This is the same computation as `karios_amd.matcher.KLT` + `ZNCCService` (reference
`karios/matcher/klt.py:198-349`, `karios/api/core.py:871-907`); only the place where the
pixels live differs.  Device buffers may come from `libkarios_hip` (`upload`) or be any
device pointer, e.g. a torch CUDA tensor's `data_ptr()` (`from_device_pointers`).

One module per concern; callers import the names below from this package.
"""
from __future__ import annotations

from .. import _lib
from .._lib import KariosHipError
from . import shared
from .buffers import DeviceBuffer
from .pair import ResidentPair
from .pending import PendingBatch, PendingFrame, RawFrame
from .scores import MI_SEARCH_COLUMNS, ZNCC_SEARCH_COLUMNS, mi_search_columns, search_columns
from .shared import forget_shared_pairs, invalidate_raster, keep_shared_across, shared_pair
from .tiles import submit_units


def __getattr__(name):
    if name == "shared_pair_uploads":          # a counter: always `shared`'s current value, never a copy made at import
        return shared.shared_pair_uploads
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["ResidentPair", "DeviceBuffer", "RawFrame", "PendingFrame", "PendingBatch", "submit_units", "shared_pair", "keep_shared_across",
           "invalidate_raster", "forget_shared_pairs", "ZNCC_SEARCH_COLUMNS", "search_columns", "KariosHipError", "_lib"]
