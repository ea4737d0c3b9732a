"""SIFT of the align step (csrc/api_sift.hip)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Context
from ._place import Place, _ctx, _raster_arg
from .match import DESCRIPTOR_DIM

SIFT_KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                                ("response", np.float32), ("octave", np.int32)])
SIFT_FIELDS = SIFT_KEYPOINT_DTYPE.names


def _sift_stats(stats):
    n = int(stats[0])
    per = [int(v) for v in stats[4:4 + 3 * n]]
    return {"octaves": n, "before_dedup": int(stats[1]), "after_dedup": int(stats[2]), "workspace_bytes": int(stats[3]),
            "candidates": per[0::3], "refined": per[1::3], "keypoints": per[2::3]}


SIFT_STAGES = ("blur_dog", "scan", "refine", "orient", "describe")


def _sift_times(stats):
    """Microseconds: device time per stage and octave (between stream events), host time of the final order and of the call."""
    n = int(stats[0])
    out = {"base": int(stats[52]), "sort_host": int(stats[53]), "gather": int(stats[54]), "call_host": int(stats[55])}
    for k, name in enumerate(SIFT_STAGES):
        out[name] = [int(stats[56 + 5 * o + k]) for o in range(n)]
    return out

def sift_capacity_estimate(H, W):
    """Room the first call gives the outputs: one key point per 16 pixels (textures measure one per 30 to 40) and a little."""
    return H * W // 16 + 256


def sift_detect_and_compute(image, *, contrast_threshold: float = 0.02, edge_threshold: float = 10, n_octave_layers: int = 3,
                            sigma: float = 1.6, descriptor_dtype=np.float32, return_stats: bool = False, capacity: int | None = None,
                            ctx: Context | None = None):
    """cv2.SIFT_create(nfeatures=0, nOctaveLayers=, contrastThreshold=, edgeThreshold=, sigma=).detectAndCompute(image, None)
    (global_align.py:48-50, 160-166) -> (key points, descriptors [n, 128] of descriptor_dtype: uint8 or float32, the same integers).
    A uint8 numpy image (rows contiguous, a row stride is fine) gives a structured array of SIFT_KEYPOINT_DTYPE and a numpy array;
    a uint8 torch tensor on the context's device gives a dict of device tensors keyed by SIFT_FIELDS and a device tensor - nothing
    but the count and the records of the final order travel to the host.  The outputs are sized by an estimate (`capacity`
    overrides it: the result is then the first `capacity` key points of the final order, and only the stats' count tells that
    there are more); when there are more key points than the estimate the call is repeated once with room for all of them.
    return_stats adds a dict: octaves, candidates / refined / keypoints per octave, before_dedup, after_dedup, workspace_bytes, count, times_us (microseconds per stage), regrows (candidate list, key-point list), calls."""
    ddt = np.dtype(descriptor_dtype)
    if ddt != np.uint8 and ddt != np.float32:
        raise ValueError(f"sift_detect_and_compute: descriptor_dtype {ddt} (uint8 or float32)")
    place = Place((image,))
    if place.dev:
        if place.dtype(image) != np.uint8 or image.dim() != 2 or (image.shape[1] > 1 and image.stride(1) != 1):
            raise ValueError("sift_detect_and_compute: expected a 2-D uint8 tensor with contiguous rows")
    else:
        image = np.asarray(image)
        if image.dtype != np.uint8:
            raise ValueError(f"sift_detect_and_compute: expected a uint8 image, got {image.dtype}")
    img_arg, _, H, W, stride = _raster_arg(place, image, "sift_detect_and_compute")
    if H < 1 or W < 1:
        raise ValueError(f"sift_detect_and_compute: empty image {H} x {W}")
    c = _ctx(ctx)                                                  # after the argument checks: they need no device
    fn, what = place.function(c, "km_sift_detect_and_compute")
    cap = int(capacity) if capacity is not None else sift_capacity_estimate(H, W)
    count = C.c_int(0)
    stats = (C.c_int64 * 160)()
    code = _lib._DTYPES[ddt]
    for attempt in range(2):
        fields = place.empty((6, max(cap, 1)), np.float32)
        desc = place.empty((max(cap, 1), DESCRIPTOR_DIM), ddt)
        rc = fn(c.handle, img_arg, H, W, stride, 0, int(n_octave_layers), float(contrast_threshold), float(edge_threshold), float(sigma),
                cap, *(place.pointer(fields[k]) for k in range(6)), place.pointer(desc), code, DESCRIPTOR_DIM, C.byref(count), stats)
        if rc == _lib.E_CAPACITY and attempt == 0 and capacity is None:
            cap = count.value
            continue
        if rc != _lib.E_CAPACITY:
            c.check(rc, what)
        break
    n = min(count.value, cap)
    kp = {} if place.dev else np.empty(n, SIFT_KEYPOINT_DTYPE)
    for k, name in enumerate(SIFT_FIELDS[:5]):
        kp[name] = fields[k, :n]
    kp["octave"] = place.view(fields[5, :n], np.int32)
    out = (kp, desc[:n])
    if return_stats:
        st = _sift_stats(stats)
        st["count"] = count.value
        st["times_us"] = _sift_times(stats)
        st["regrows"] = (int(stats[136]), int(stats[137]))
        st["calls"] = attempt + 1
        out += (st,)
    return out
