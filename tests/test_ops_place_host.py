"""CPU suite: the `_place` module of `karios_amd.ops` - the one place that says whether a call's arrays are numpy arrays or torch tensors - and the
argument helpers built on it, with numpy arrays and with CPU tensors (which have `data_ptr`, so they take the tensor branch).  No
library call is made and nothing is synchronised: pointers, strides in elements, types, shapes and the refusals are what is checked,
at the smallest sizes where a rule of the marshalling can go wrong.  The second part pins the public names of `karios_amd.ops`."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from karios_amd import ops
from karios_amd.ops import _place as P

KINDS = ("numpy", "tensor")


def make(kind, a):
    return a if kind == "numpy" else torch.from_numpy(a)


def address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def value(p):
    return C.cast(p, C.c_void_p).value


# ---- Place ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_place_answers_for_one_array(kind):
    a = make(kind, np.arange(80, dtype=np.int16).reshape(8, 10))
    place = P.Place((None, a))
    assert place.dev == (kind == "tensor") and (place.device is None) == (kind == "numpy")
    assert place.holds(a) and not place.holds(make("tensor" if kind == "numpy" else "numpy", np.zeros(2)))
    window = a[2:6, 3:9]
    assert value(place.pointer(window)) == place.address(window) == address(a) + 2 * (2 * 10 + 3)
    assert place.pointer(None) is None and place.address(None) is None
    assert place.strides(a) == (10, 1) and place.strides(window) == (10, 1) and place.strides(window.T) == (1, 10)
    assert place.dtype(a) == np.dtype("int16")
    host = place.to_host(window)
    assert type(host) is np.ndarray and np.array_equal(host, np.arange(80).reshape(8, 10)[2:6, 3:9])
    seen = place.view(a, np.uint16)
    assert place.dtype(seen) == np.dtype("uint16") and address(seen) == address(a)


def test_place_of_nothing_is_the_host():
    place = P.Place(())
    assert not place.dev and place.device is None and type(place.empty(2, np.uint8)) is np.ndarray


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["uint8", "int8", "int32", "float32", "float64"])
def test_empty_gives_the_type_and_shape_where_the_arrays_live(kind, dtype):
    place = P.Place((make(kind, np.zeros(1, np.float32)),))
    for shape in (0, 3, (2, 3), (3, 4, 5)):
        out = place.empty(shape, dtype)
        assert place.holds(out) and place.dtype(out) == np.dtype(dtype)
        assert tuple(out.shape) == (shape if isinstance(shape, tuple) else (shape,))
        if kind == "tensor":
            assert out.device == place.device


@pytest.mark.parametrize("first", KINDS)
def test_a_mixed_call_is_refused_in_the_wrappers_words(first):
    a, b = make(first, np.zeros(3, np.float32)), make("tensor" if first == "numpy" else "numpy", np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="^ce_figure: dx, dy and score must all be numpy arrays or all be device tensors$"):
        P.Place((a, a, b), "ce_figure", "dx, dy and score")
    with pytest.raises(ValueError, match="^sigma_clip_batch: all columns must be numpy arrays or all be device tensors$"):
        P.Place((a, b), "sigma_clip_batch", refusal="all columns must be numpy arrays or all be device tensors")
    with pytest.raises(ValueError, match="^extract_chips: rasters and columns must all be numpy arrays or all be device tensors$"):
        P.Place((a,)).require((a, b), "extract_chips", "rasters and columns")
    with pytest.raises(ValueError, match="^box_stats: values and positions must all be numpy arrays or all be device tensors$"):
        P._f32_columns((a, b), "box_stats", "values and positions")


def test_the_wrappers_refuse_a_mixed_call_without_a_device():
    col, t = np.zeros(3, np.float32), torch.zeros(3)
    with pytest.raises(ValueError, match="accuracy_statistics: dx, dy and score must all be"):
        ops.accuracy_statistics(col, t, col, 0.5)
    with pytest.raises(ValueError, match="sample_points: raster and columns must all be"):
        ops.sample_points(torch.zeros((4, 6)), col, col)
    with pytest.raises(ValueError, match="sigma_clip_batch: all columns must be numpy arrays or all be device tensors"):
        ops.sigma_clip_batch([(col, t)])
    with pytest.raises(ValueError, match="find_homography: device points must be float32 tensors of shape \\[n, 2\\]"):
        ops.find_homography(torch.zeros((4, 2)), np.zeros((4, 2), np.float32), ctx=object())
    with pytest.raises(ValueError, match="point_rasters: the output must live where the columns live"):
        ops.point_rasters(col, col, shape=(4, 6), out_mask=torch.zeros((4, 6), dtype=torch.uint8))


# ---- columns -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 3])
def test_columns_of_n_rows(kind, n):
    cols = tuple(make(kind, np.arange(n, dtype=np.float32) + k) for k in range(3))
    place, got, rows = P._f32_columns(cols, "w", "a, b and c")
    assert rows == n and place.dev == (kind == "tensor") and all(g is c for g, c in zip(got, cols))
    args = P._col_args(place, got, rows)
    assert args == [None] * 3 if n == 0 else [value(p) for p in args] == [address(c) for c in cols]
    assert P._float32_columns(place, cols)[1]


@pytest.mark.parametrize("kind", KINDS)
def test_columns_that_the_library_cannot_read(kind):
    f, d = make(kind, np.zeros(6, np.float32)), make(kind, np.zeros(6, np.float64))
    shape = "contiguous 1-D float32 tensors" if kind == "tensor" else "1-D float32 arrays"
    for cols in ((f, d), (f, f.reshape(2, 3))):
        assert not P._float32_columns(P.Place(cols), cols)[1]
        with pytest.raises(ValueError, match=f"^w: a and b must be {shape}$"):
            P._f32_columns(cols, "w", "a and b")
    with pytest.raises(ValueError, match="^w: a and b differ in length$"):
        P._f32_columns((f, f[:5]), "w", "a and b")
    place = P.Place((f,))
    strided = f[::2]
    if kind == "tensor":        # a strided tensor is refused, a strided numpy column is copied
        assert not P._float32_columns(place, (strided,))[1]
    else:
        (got,), rows = P._f32_columns((strided,), "w", "a")[1:]
        assert rows == 3 and got.flags.c_contiguous and got is not strided


# ---- rasters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (4, 6)])
def test_raster_of_a_shape(kind, shape):
    a = make(kind, np.arange(shape[0] * shape[1], dtype=np.uint16).reshape(shape))
    arg, dt, H, W, stride = P._raster_arg(P.Place((a,)), a, "w")
    assert (value(arg), dt, H, W, stride) == (address(a), np.dtype("uint16"), shape[0], shape[1], shape[1])


@pytest.mark.parametrize("kind", KINDS)
def test_raster_windows_of_a_wider_buffer(kind):
    buf = make(kind, np.arange(80, dtype=np.float32).reshape(8, 10))
    place = P.Place((buf,))
    for window, origin, want in ((buf[1:5, 2:8], 12, 10), (buf[3:4, 2:8], 32, 6), (buf[1:5, 4:5], 14, 10)):   # 4 x 6; one row: W; one column
        arg, dt, H, W, stride = P._raster_arg(place, window, "w")
        assert (value(arg), stride) == (address(buf) + 4 * origin, want) and (H, W) == tuple(window.shape) and dt == np.float32


def test_a_transposed_raster_is_refused_for_tensors_and_copied_for_numpy():
    a = np.arange(24, dtype=np.uint8).reshape(6, 4)
    with pytest.raises(ValueError, match="^w: expected a 2-D tensor with contiguous rows$"):
        P._raster_arg(P.Place((torch.from_numpy(a),)), torch.from_numpy(a).T, "w")
    with pytest.raises(ValueError, match="^w: expected a 2-D tensor with contiguous rows$"):
        P._raster_arg(P.Place((torch.from_numpy(a),)), torch.from_numpy(a)[0], "w")
    arg, dt, H, W, stride = P._raster_arg(P.Place((a,)), a.T, "w")
    assert (H, W, stride) == (4, 6, 6) and value(arg) != a.ctypes.data
    assert (C.c_uint8 * 24).from_address(value(arg))[:] == list(a.T.ravel())
    one_column = torch.from_numpy(a).T[:, :1]             # a one-column raster's column stride is not examined
    assert P._raster_arg(P.Place((one_column,)), one_column, "w")[2:] == (4, 1, 1)


def test_the_dtype_override_of_a_tensors_storage_checks_the_item_size():
    t = torch.zeros((4, 6), dtype=torch.int16)
    place = P.Place((t,))
    assert P._raster_arg(place, t, "w", np.uint16)[1] == np.dtype("uint16")
    assert P._raster_arg(place, t, "w", "int16")[1] == np.dtype("int16")
    with pytest.raises(ValueError, match="^w: pixel type float32 in int16 storage$"):
        P._raster_arg(place, t, "w", np.float32)
    with pytest.raises(ValueError, match="^w: pixel type uint8 in int16 storage$"):
        P._raster_arg(place, t, "w", np.uint8)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def test_masks_of_a_numpy_raster():
    place = P.Place((np.zeros((4, 6), np.uint8),))
    assert P._mask_arg(place, None, 4, 6, "w") == (None, 0)
    u8 = np.zeros((8, 10), np.uint8)[2:6, 1:7]
    arg, stride = P._mask_arg(place, u8, 4, 6, "w")
    assert (value(arg), stride) == (u8.ctypes.data, 10)
    pattern = np.arange(24).reshape(4, 6) % 3
    for m in (pattern != 0, (pattern * 300).astype(np.int32), -pattern.astype(np.float32)):      # not uint8: (m != 0)
        arg, stride = P._mask_arg(place, m, 4, 6, "w")
        assert stride == 6 and (C.c_uint8 * 24).from_address(value(arg))[:] == list((pattern != 0).ravel().astype(int))
    with pytest.raises(ValueError, match="^w: mask shape differs from the raster's$"):
        P._mask_arg(place, np.zeros((6, 4), np.uint8), 4, 6, "w")


def test_masks_of_a_tensor_raster():
    place = P.Place((torch.zeros((4, 6)),))
    assert P._mask_arg(place, None, 4, 6, "w") == (None, 0)
    buf = torch.zeros((8, 10), dtype=torch.uint8)
    arg, stride = P._mask_arg(place, buf[2:6, 1:7], 4, 6, "w")
    assert (value(arg), stride) == (buf.data_ptr() + 21, 10)
    assert P._mask_arg(P.Place((buf,)), buf[2:3, 1:7], 1, 6, "w")[1] == 6           # one row: W
    refusal = "^w: the mask must be a uint8 tensor of the raster's shape with contiguous rows$"
    for bad in (torch.zeros((4, 6), dtype=torch.bool), torch.zeros((4, 6), dtype=torch.int32), torch.zeros((6, 4), dtype=torch.uint8),
                torch.zeros((6, 4), dtype=torch.uint8).T, np.zeros((4, 6), np.uint8)):
        with pytest.raises(ValueError, match=refusal):
            P._mask_arg(place, bad, 4, 6, "w")


# ---- output planes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_output_planes(kind):
    place = P.Place((make(kind, np.zeros(1, np.float32)),))
    fresh = P._out_plane(place, None, (2, 4, 6), np.float32, "w")
    assert place.holds(fresh) and tuple(fresh.shape) == (2, 4, 6) and place.dtype(fresh) == np.float32
    buf = make(kind, np.zeros((8, 10), np.uint8))
    window = buf[1:5, 2:8]
    assert P._out_plane(place, window, (4, 6), np.uint8, "w") is window
    refusal = "^w: the output must be a writable uint8 buffer of shape \\(4, 6\\) with contiguous rows$"
    for bad in (make(kind, np.zeros((4, 6), np.int8)), make(kind, np.zeros((6, 4), np.uint8)), make(kind, np.zeros((6, 4), np.uint8)).T):
        with pytest.raises(ValueError, match=refusal):
            P._out_plane(place, bad, (4, 6), np.uint8, "w")
    if kind == "numpy":
        frozen = np.zeros((4, 6), np.uint8)
        frozen.flags.writeable = False
        with pytest.raises(ValueError, match=refusal):
            P._out_plane(place, frozen, (4, 6), np.uint8, "w")
    with pytest.raises(ValueError, match="^w: the output must live where the columns live$"):
        P._out_plane(place, make("tensor" if kind == "numpy" else "numpy", np.zeros((4, 6), np.uint8)), (4, 6), np.uint8, "w")


# ---- the public names ----------------------------------------------------------------------------------------------------------------
PUBLIC = [
    "ACCURACY_MAX_ROWS", "ACCURACY_STAT_NAMES", "AccuracyStatistics", "BOX_STAT_NAMES", "BoxStats", "C", "CE_FIELDS", "CE_MAX_BINS",
    "CHIP_KSIZES", "CHIP_SIZE", "CLIP_MAX_ROWS", "CeFigure", "ChipImages", "Context", "DESCRIPTOR_DIM", "DISPLAY_MAX_NO_VALUES",
    "DisplayRange", "EXCLUDE_NAN", "EXCLUDE_NONFINITE", "INTER_LINEAR", "INTER_NEAREST", "KariosHipError", "KltParams", "PREP_DTYPES",
    "PROFILE_MAX", "PROFILE_MAX_BIN", "PROFILE_MAX_ROWS", "ProfileColumns", "RANSAC_STATS", "SIFT_FIELDS", "SIFT_KEYPOINT_DTYPE",
    "SIFT_STAGES", "TERM_CRITERIA_COUNT", "TERM_CRITERIA_EPS", "WARP_INVERSE_MAP", "accuracy_statistics", "annotations", "as_image",
    "auto_mask", "box_stats", "calc_optical_flow_pyr_lk", "ce_figure", "chip_ksize", "clahe", "count_valid_pixels", "default_context",
    "display_range", "dtype_code", "ecc_stages", "extract_chips", "find_homography", "find_transform_ecc", "frame_from_tracks",
    "good_features_to_track", "klt_tile", "klt_track", "knn_match", "laplacian_u8", "lerp_linear", "lk_oscillation_probe", "make_params",
    "match_lowe_mutual", "mean_profiles", "mi_batch", "min_eigen", "nanpercentile", "np", "order_statistics", "percentile",
    "phase_cross_correlation", "point_rasters", "preprocess", "ptr", "pyr_down", "refine_ecc_candidates", "row_stride", "sample_points",
    "select_chip_points", "shift_image", "sift_capacity_estimate", "sift_detect_and_compute", "sigma_clip", "sigma_clip_batch",
    "sobel_magnitude", "stretch_percentile_u8", "tile_prefilter", "to_uint8", "to_uint8_percentile", "warp_perspective", "zncc_batch",
    "zncc_windows"]
PATCHED = {"accuracy_statistics": "accuracy", "find_homography": "match", "refine_ecc_candidates": "align", "warp_perspective": "align",
           "sobel_magnitude": "align", "sift_detect_and_compute": "sift"}


def test_the_public_names_of_ops_resolve():
    """The names without a leading underscore of the single-file `ops` this package replaced, and the module `tests/conftest.py` reads."""
    assert [name for name in PUBLIC if not hasattr(ops, name)] == []
    assert ops._lib is importlib.import_module("karios_amd._lib")
    namespace = {}
    exec("from karios_amd.ops import " + ", ".join(PUBLIC), namespace)
    assert all(namespace[name] is getattr(ops, name) for name in PUBLIC)


def test_the_names_the_host_tests_replace_are_the_modules_own():
    """`monkeypatch.setattr(ops, NAME, ...)` reaches every caller as long as `ops.NAME` is the one function and nothing inside the
    package calls it by another path."""
    for name, module in PATCHED.items():
        assert getattr(ops, name) is getattr(importlib.import_module(f"karios_amd.ops.{module}"), name)
