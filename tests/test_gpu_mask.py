"""GPU suite: vector masks on the device (csrc/k_mask.hip) - the polygon burn of rasterize_vector_mask and the AND of _load_mask - held
byte for byte to their definition, tests/rasterize_restatement.py, on the shared case list (tests/mask_cases.py).  No recorded GDAL
results exist (GDAL is installed nowhere this project is tested); what the definition itself is checked against: tests/test_mask_host.py."""
import json

import numpy as np
import pytest

import mask_cases as M
import rasterize_restatement as R

from karios_amd import ops, results, synth  # noqa: E402
from karios_amd.core import DeviceRasterImage, KLTConfiguration, NumpyRasterImage, rasterize_vector_mask  # noqa: E402
from karios_amd.matcher import KLT  # noqa: E402
from test_gpu_report import to_dev, to_host  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = M.cases()
FORMS = ("numpy", "device")


@pytest.fixture(scope="module")
def expected():
    return {name: R.rasterize(features, H, W) for name, features, H, W, _options in CASES}


def burn(form, features, H, W, window):
    """-> (the raster as a host array, the host copy of the whole buffer it was written into, the window's slices)."""
    import torch
    rows, cols = (slice(2, 2 + H), slice(3, 3 + W)) if window else (slice(0, H), slice(0, W))
    shape = (H + 3, W + 24) if window else (H, W)
    if form == "device":
        buf = torch.full(shape, 0xAB, dtype=torch.uint8, device="cuda")
        out = ops.rasterize_polygons(features, (H, W), out=buf[rows, cols])
        assert out.data_ptr() == buf[rows, cols].data_ptr()
        whole = buf.cpu().numpy()
    elif window:
        whole = np.full(shape, 0xAB, np.uint8)
        ops.rasterize_polygons(features, (H, W), out=whole[rows, cols])
    else:
        whole = ops.rasterize_polygons(features, (H, W))
        assert isinstance(whole, np.ndarray) and whole.dtype == np.uint8
    return whole[rows, cols], whole, (rows, cols)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cases_equal_the_restatement(ops, expected, form, case):
    name, features, H, W, options = case
    ctx = ops.default_context()
    ctx.set_option("mask_edge_chunk", options.get("chunk", 0))
    try:
        got, whole, (rows, cols) = burn(form, features, H, W, options.get("window", False))
    finally:
        ctx.set_option("mask_edge_chunk", 0)
    want = expected[name]
    assert got.shape == want.shape and np.array_equal(got, want), (name, np.argwhere(got != want)[:8])
    whole = whole.copy()
    whole[rows, cols] = 0xAB
    assert (whole == 0xAB).all(), name                               # nothing outside the window


def test_device_argument_puts_the_result_on_the_device(ops, expected):
    import torch
    name, features, H, W, _options = CASES[0]
    out = ops.rasterize_polygons(features, (H, W), device=torch.device("cuda"))
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), expected[name])


def test_two_calls_give_identical_bytes(ops, expected):
    import torch
    for name in ("45x67", "random_many", "3x4099"):
        _n, features, H, W, _o = next(c for c in CASES if c[0] == name)
        stale = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")          # whatever the buffer held before must not matter
        a = ops.rasterize_polygons(features, (H, W), out=stale).cpu().numpy().copy()
        b = ops.rasterize_polygons(features, (H, W), device="cuda").cpu().numpy()
        c = ops.rasterize_polygons(features, (H, W))
        assert a.tobytes() == b.tobytes() == c.tobytes() == expected[name].tobytes(), name


@pytest.mark.parametrize("form", FORMS)
def test_combine_masks_equals_numpy(ops, form):
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (7, 33), (64, 64), (45, 67), (3, 4099)):
        a = (rng.integers(0, 4, (H, W)) * rng.integers(0, 90, (H, W))).astype(np.uint8)       # values above 1
        b = (rng.integers(0, 3, (H, W)) * 255).astype(np.uint8)
        want, want_counts = R.combine_masks(a, b)
        if form == "device":
            wide_a, wide_b = np.zeros((H + 1, W + 21), np.uint8), np.zeros((H, W + 5), np.uint8)
            wide_a[1:, 3:3 + W], wide_b[:, 5:] = a, b
            got, counts = ops.combine_masks(to_dev(wide_a)[1:, 3:3 + W], to_dev(wide_b)[:, 5:])                     # windows, off the 16-byte grid
            got2, counts2 = ops.combine_masks(to_dev(a), to_dev(b))
            assert np.array_equal(to_host(got2), want) and counts2 == want_counts
        else:
            got, counts = ops.combine_masks(a, b)
        assert np.array_equal(to_host(got), want) and counts == want_counts, (H, W)
        assert all(isinstance(c, int) for c in counts)
    if form == "numpy":
        got, counts = ops.combine_masks(np.array([[0, 3, -2]], np.int16), np.array([[1.5, 0.25, 7.0]]))                # any host dtype: > 0
        assert got.tolist() == [[0, 1, 0]] and counts == (1, 3, 1)


AOI = [[16.0, 100.0], [40.5, 20.25], [110.0, 12.0], [120.5, 90.0], [70.0, 118.5], [16.0, 100.0]]      # world coordinates, y up
GT = [0.0, 1.0, 0.0, 128.0, 0.0, -1.0]


def test_vector_mask_goes_into_klt_match_from_the_device(ops, tmp_path):
    """rasterize_vector_mask on a DeviceRasterImage gives a DeviceRasterImage KLT.match takes as its mask; the frame equals the one
    obtained with the same mask - the definition's bytes - uploaded from the host."""
    import torch
    mon_t, ref_t = synth.make_pair_torch(128, 128, 0.4, -0.2, seed=4, device=torch.device("cuda"))
    torch.cuda.synchronize()
    mon, ref = DeviceRasterImage(mon_t, np.uint16), DeviceRasterImage(ref_t, np.uint16)
    doc = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [AOI]}}]}
    path = tmp_path / "aoi.geojson"
    path.write_text(json.dumps(doc))
    mask = rasterize_vector_mask(path, mon, geo_transform=GT)
    assert isinstance(mask, DeviceRasterImage) and mask.tensor.is_cuda and (mask.y_size, mask.x_size) == (128, 128)
    want = R.rasterize([[R.geo_to_pixel(AOI, GT)]], 128, 128)
    assert np.array_equal(mask.tensor.cpu().numpy(), want) and 0 < int(want.sum()) < 128 * 128
    conf = KLTConfiguration(tile_size=128, maxCorners=400, laplacian_kernel_size=5)
    frames = list(KLT(conf).match(mon, ref, mask))
    uploaded = list(KLT(conf).match(mon, ref, DeviceRasterImage(to_dev(want))))
    assert len(frames) == len(uploaded) == 1 and len(frames[0]) > 10
    assert frames[0].equals(uploaded[0]) and list(frames[0].columns) == list(uploaded[0].columns)
    inside = want[frames[0]["y0"].to_numpy().astype(int), frames[0]["x0"].to_numpy().astype(int)]
    assert inside.all()                                              # every key point lies under the mask
    # a host image gives a host mask; a features list in pixel space is taken as it is; a parsed dict equals the file
    host = rasterize_vector_mask(doc, NumpyRasterImage(np.zeros((128, 128), np.uint16)), geo_transform=GT)
    assert isinstance(host, NumpyRasterImage) and np.array_equal(host.array, want)
    assert np.array_equal(rasterize_vector_mask([[R.geo_to_pixel(AOI, GT)]], mon).tensor.cpu().numpy(), want)


def test_load_mask_mirrors_the_reference(ops, caplog):
    import logging
    import torch
    rng = np.random.default_rng(8)
    raster = (rng.integers(0, 3, (128, 128)) * 100).astype(np.uint8)
    want_vector = R.rasterize([[R.geo_to_pixel(AOI, GT)]], 128, 128)
    want, counts = R.combine_masks(raster, want_vector)
    doc = {"type": "Polygon", "coordinates": [AOI]}
    mon_dev = DeviceRasterImage(torch.zeros((128, 128), dtype=torch.int16, device="cuda"), np.uint16)
    mon_host = NumpyRasterImage(np.zeros((128, 128), np.uint16))
    line = "Mask combination: raster=%d valid pixels, vector=%d valid pixels, combined=%d valid pixels (AND logic)" % counts
    for mon, raster_image in ((mon_dev, DeviceRasterImage(to_dev(raster))), (mon_dev, NumpyRasterImage(raster)), (mon_host, NumpyRasterImage(raster))):
        with caplog.at_level(logging.INFO, logger="karios_amd.results"):
            caplog.clear()
            both = results.load_mask(mon, raster_mask=raster_image, vector=doc, geo_transform=GT)
        assert isinstance(both, DeviceRasterImage if mon is mon_dev else NumpyRasterImage)
        assert np.array_equal(to_host(both.tensor) if mon is mon_dev else both.array, want)
        assert line in [r.getMessage() for r in caplog.records]
    only = results.load_mask(mon_dev, vector=doc, geo_transform=GT)
    assert isinstance(only, DeviceRasterImage) and np.array_equal(only.tensor.cpu().numpy(), want_vector)
