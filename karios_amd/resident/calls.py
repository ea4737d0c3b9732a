"""What the tile and score calls of a resident pair share: one rule each for a frame's capacity and its score columns, the no-data
pointers, and the context state a call runs under (`Scope`)."""
from __future__ import annotations

import ctypes as C


def frame_capacity(max_corners: int, x_size: int, y_size: int) -> int:
    """Rows the frame block of a box holds: maxCorners, or a quarter of the box's pixels without a limit."""
    return max_corners if max_corners > 0 else max(1, (x_size * y_size) // 4)


def score_columns(zncc_threshold, mutual_info: bool = False) -> int:
    """float64 score columns behind a frame's six float32 ones (`frames.block_words`): 0 without a threshold, 1 `zncc_score`, 3 with
    `mutual_info` (zncc_score | mutual_info_score | mi_score)."""
    return 0 if zncc_threshold is None else (3 if mutual_info else 1)


def clips(conf) -> bool:
    """The configuration asks for the tracker's outlier clip (klt.py:52-71)."""
    return bool(getattr(conf, "outliers_filtering", False))


def no_data_pointers(pair):
    """(nodata_ref, nodata_mon) as the library takes them: a pointer to the value, NULL without one."""
    nr = C.byref(C.c_double(float(pair.no_data_ref))) if pair.no_data_ref is not None else None
    nm = C.byref(C.c_double(float(pair.no_data_mon))) if pair.no_data_mon is not None else None
    return nr, nm


class Scope:
    """Context manager for the context state one call runs under, set in this order and reset in reverse, also when the call raises:
    `window` - the ZNCC / MI kernels see this image window (km_set_image_window; None: the buffers are the image);
    `mi` - frames scored inside also carry `mutual_info_score` / `mi_score` (km_set_option "frame_mi");
    `clip` - frames produced inside are clipped by the tracker's outlier filter on the device, in front of their scores
    (km_set_option "frame_clip").  The library reads the values when the call is made, so a pipelined submission keeps them.
    What is off is not touched."""
    __slots__ = ("ctx", "window", "mi", "clip", "entered")

    def __init__(self, ctx, window=None, mi: bool = False, clip: bool = False):
        self.ctx, self.window, self.mi, self.clip, self.entered = ctx, window, mi, clip, 0

    def __enter__(self):
        c = self.ctx
        try:
            if self.window is not None:
                c.check(c.lib.km_set_image_window(c.handle, *(int(v) for v in self.window)), "km_set_image_window")
            self.entered = 1
            if self.mi:
                c.set_option("frame_mi", 1)
            self.entered = 2
            if self.clip:
                c.set_option("frame_clip", 1)
            self.entered = 3
        except BaseException:
            self.__exit__()            # (a set call failed: what was set before it is reset, nothing else)
            raise
        return self

    def __exit__(self, *exc):
        c = self.ctx
        try:
            if self.clip and self.entered >= 3:
                c.set_option("frame_clip", 0)
        finally:
            try:
                if self.mi and self.entered >= 2:
                    c.set_option("frame_mi", 0)
            finally:
                if self.window is not None and self.entered >= 1:
                    c.lib.km_set_image_window(c.handle, 0, 0, 0, 0)
        return False
