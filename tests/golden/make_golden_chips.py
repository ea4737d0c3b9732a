#!/usr/bin/env python3
"""Golden vectors for the key-point chips, produced by the REFERENCE's own `CenterAndQuarterCellPointSelector.select_points` and
`ChipService._to_chips_gdal_dataset` (karios/report/chip_service.py), imported from /root/reference (build container only).

Run here, never on the GPU box:   python tests/golden/make_golden_chips.py      -> tests/golden/chips.npz
Only DATA is written: checksums of the input columns (rebuilt by `selection_cases` below, integer arithmetic only), the selected
row indices, the text of one chips.csv, and for the chip cases which rows were written, their names and their uint8 / Laplacian
arrays.  No reference source is copied.

The reference's chip routine runs as it is, with stand-ins in its module namespace for what this environment lacks: an
array-backed dataset, `gdal.Translate` cutting `srcWin`, `cv2.imwrite` capturing the array, `cv2.Laplacian` = the CPU oracle.

`selection_cases`, `chip_cases` and the lists below are imported by the tests; nothing at module level touches the reference.
"""
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_accuracy import _hash, _unit  # noqa: E402

f32 = np.float32
THRESHOLD = 0.4
T32 = f32(THRESHOLD)
ULP_ROWS = (T32, np.nextafter(T32, f32(1)), np.nextafter(T32, f32(0)))
DTYPES = ("uint8", "uint16", "int16", "float32")
KSIZES = ({"ref": 1, "mon": 1}, {"ref": 3, "mon": 3}, {"ref": 5, "mon": 5}, {"ref": 7, "mon": 7}, {"ref": 9, "mon": 9},
          {"ref": 11, "mon": 11}, {"ref": 11, "mon": 7}, {"mon": 5}, None)
# a threshold between float32(0.4) and the next float32: as a Python float it compares in float32 (a score AT float32(0.4) passes), as an
# np.float64 in float64 (that score fails)
THRESHOLD_HI = 0.40000001
THRESHOLDS = (("py", THRESHOLD), ("f64", np.float64(THRESHOLD)), ("py_hi", THRESHOLD_HI), ("f64_hi", np.float64(THRESHOLD_HI)))
CSV_CASE = "rows26"


def crc(*arrays):
    v = 0
    for a in arrays:
        v = zlib.crc32(np.ascontiguousarray(a).tobytes(), v)
    return v


def _frame(n, seed, width, height, integer=True):
    """x0, y0 inside the image (integer valued like the tracker's corners unless `integer` is off), scores on a grid of 1 / 64."""
    x = _unit(n, 5 * seed + 1) * width
    y = _unit(n, 5 * seed + 2) * height
    if integer:
        x, y = np.floor(x), np.floor(y)
    score = ((_hash(n, 5 * seed + 3) % np.uint64(65)).astype(f32)) / f32(64)
    return x.astype(f32), y.astype(f32), score


def selection_cases():
    """-> list of (name, x0, y0, score, width, height): float32 columns, rebuilt identically everywhere."""
    out = []
    for k, n in enumerate((1, 2, 5, 26)):
        x, y, s = _frame(n, k, 640, 403)
        s[:] = np.maximum(s, f32(0.5))
        out.append((f"rows{n}", x, y, s, 640, 403))
    # all rows in one cell (cell 12 of 640 x 403), not integer valued
    x, y, s = _frame(40, 10, 128, 80.6, integer=False)
    out.append(("one_cell", x + f32(256), y + f32(161.2), s, 640, 403))
    # one row per cell
    cx, cy = np.meshgrid(np.arange(5), np.arange(5))
    x = (cx.ravel() * 128 + 17 + (_hash(25, 21) % np.uint64(90)).astype(np.int64)).astype(f32)
    y = (cy.ravel() * 80 + 9 + (_hash(25, 22) % np.uint64(60)).astype(np.int64)).astype(f32)
    out.append(("per_cell", x, y, np.full(25, 0.75, f32), 640, 403))
    out.append(("grid_403x640",) + _frame(1000, 30, 640, 403) + (640, 403))
    out.append(("grid_10980",) + _frame(20000, 31, 10980, 10980) + (10980, 10980))
    # duplicate positions, distance ties with different scores, ties in distance and score: few positions, few score levels
    x, y, s = _frame(400, 40, 64, 64)
    s = ((_hash(400, 41) % np.uint64(4)).astype(f32) + f32(4)) / f32(8)
    out.append(("ties", np.floor(x / 4) * 4, np.floor(y / 4) * 4, s, 64, 64))
    # rows exactly on x_end / y_end of the last column / row, beside ordinary rows of those cells
    x, y, s = _frame(300, 50, 640, 403)
    s[:] = np.maximum(s, f32(0.5))
    x[::7], y[::11] = f32(640), f32(403)
    x[5], y[5] = f32(640), f32(403)
    out.append(("on_end", x, y, s, 640, 403))
    # scores at float32(0.4), one ulp above and one below, each the row nearest to a cell centre
    x, y, s = _frame(200, 60, 640, 403)
    s[:] = np.maximum(s, f32(0.5))
    for j, (c, v) in enumerate(zip((0, 12, 24), ULP_ROWS)):
        x[j], y[j], s[j] = f32((c % 5) * 128 + 64), f32((c // 5) * 80.6 + 40.3), v
    out.append(("ulp", x, y, s, 640, 403))
    return out


def points_frame(x0, y0, score):
    """The frame of a selection case: its columns plus dx, dy (float32, hashed)."""
    import pandas as pd
    n = x0.size
    return pd.DataFrame({"x0": x0, "y0": y0, "dx": (_unit(n, 77) - 0.5).astype(f32), "dy": (_unit(n, 78) - 0.5).astype(f32), "score": score})


def _scene(H, W, dtype, seed):
    """A smooth synthetic scene plus noise as `dtype` (ref, mon); float32 carries NaN pixels; one 57 x 57 area of both is constant."""
    from karios_amd import synth
    mon, ref = synth.make_pair(max(H, 64), max(W, 64), 0.5, 0.0)
    out = []
    for k, img in enumerate((ref, mon)):
        a = img[:H, :W].astype(np.float64)
        a = (a - a.min()) / max(a.max() - a.min(), 1e-9)
        noise = _unit(H * W, 100 + 7 * seed + k).reshape(H, W)
        v = 0.7 * a + 0.3 * noise
        dt = np.dtype(dtype)
        if dt == np.uint8:
            r = (v * 255).astype(np.uint8)
        elif dt == np.uint16:
            r = (v * 9000 + 300).astype(np.uint16)
        elif dt == np.int16:
            r = (v * 9000 - 4000).astype(np.int16)
        else:
            r = (v * 3.5 - 1.25).astype(np.float32)
        out.append(r)
    return out


def chip_cases():
    """-> list of (name, ref, mon, x0, y0, dx, dy, list of laplacian_ksize settings)."""
    cases = []
    # every border for ref and for mon, the half-way offsets, the float32 / float64 rounding case: uint16, 97 x 131
    H, W = 97, 131
    ref, mon = _scene(H, W, "uint16", 0)
    ref[10:67, 20:77] = 1234                       # constant chips around (48, 38) of ref; mon keeps its content there
    rows = [(65, 48, 0.25, -0.25), (48, 38, 3.0, 2.0)]
    for x, y in ((28, 48), (27, 48), (W - 29, 48), (W - 28, 48), (65, 28), (65, 27), (65, H - 29), (65, H - 28)):
        rows.append((x, y, 0.0, 0.0))                                  # ref and mon touch / leave together ...
    for x, y, dx, dy in ((30, 48, -2.0, 0.0), (30, 48, -3.0, 0.0), (W - 31, 48, 2.0, 0.0), (W - 31, 48, 3.0, 0.0),
                         (65, 30, 0.0, -2.0), (65, 30, 0.0, -3.0), (65, H - 31, 0.0, 2.0), (65, H - 31, 0.0, 3.0)):
        rows.append((x, y, dx, dy))                                    # ... and mon alone
    rows += [(60, 48, 0.5, 0.5), (61, 48, 0.5, 0.5), (60, 49, -0.5, -0.5), (61, 49, -0.5, -0.5)]
    rows.append((63, 50, float(f32(0.499999)), float(f32(0.499999))))   # float32 sum 63.5 -> 64, float64 sum -> 63
    cols = [np.array(c, f32) for c in zip(*rows)]
    cases.append(("borders_uint16", ref, mon, *cols, [{"ref": 5, "mon": 3}]))
    # every pixel type: a plain chip, a constant one, half-way offsets; float32 with NaN inside the chips
    for k, dt in enumerate(DTYPES):
        ref, mon = _scene(H, W, dt, 1 + k)
        mon[30:87, 40:97] = 77 if dt != "float32" else f32(0.125)
        if dt == "float32":
            ref[40, 60] = ref[55, 70] = mon[48, 66] = np.nan
        rows = [(65, 48, 0.25, -0.25), (68, 58, 0.0, 0.0), (61, 40, 0.5, -0.5), (27, 48, 0.0, 0.0)]
        cases.append((f"types_{dt}", ref, mon, *[np.array(c, f32) for c in zip(*rows)], [{"ref": 3, "mon": 7}]))
    # every kernel-size setting on the smallest rasters
    ref, mon = _scene(57, 57, "uint8", 9)
    one = [np.array(c, f32) for c in zip((28, 28, 0.5, 0.0))]
    cases.append(("k_57x57", ref, mon, *one, list(KSIZES)))
    ref, mon = _scene(58, 57, "int16", 10)
    two = [np.array(c, f32) for c in zip((28, 28, 0.0, 0.75), (28, 29, 0.0, -0.6), (29, 28, 0.0, 0.0))]
    cases.append(("k_58x57", ref, mon, *two, [KSIZES[6], KSIZES[7], KSIZES[8]]))
    return cases


def ktag(k):
    return "none" if k is None else "_".join(f"{n}{k[n]}" for n in sorted(k))


def main():
    import pandas as pd
    from pathlib import Path
    from make_golden import import_reference
    import_reference()
    from oracle import oracle as O
    import karios.report.chip_service as rcs

    out = {}
    # ---- selections
    for name, x0, y0, score, width, height in selection_cases():
        out[f"crc_{name}"] = np.array([crc(x0, y0, score)], np.uint32)
        df = points_frame(x0, y0, score)
        df["row"] = np.arange(x0.size, dtype=f32)
        for tag, thr in THRESHOLDS:
            filtered = df[df["score"] >= thr]
            sel = rcs.CenterAndQuarterCellPointSelector(width, height).select_points(filtered)
            assert len(sel) > 0 and all(str(t) == "float64" for t in sel.dtypes), sel.dtypes
            out[f"sel_{name}_{tag}"] = sel["row"].to_numpy().astype(np.int32)
            if name == CSV_CASE and tag == "py":
                out["csv_text"] = np.array(sel.drop(columns="row").to_csv(sep=";", index=False))
    assert 0 in out["sel_ulp_py"] and 0 in out["sel_ulp_py_hi"] and 0 not in out["sel_ulp_f64_hi"] and 2 not in out["sel_ulp_f64"]

    # ---- chips: the reference's routine over stand-ins
    class Band:
        def __init__(self, a):
            self.a = a

        def ReadAsArray(self, xoff=0, yoff=0, xs=None, ys=None):
            a = self.a
            return a.copy() if xs is None else a[yoff:yoff + ys, xoff:xoff + xs].copy()

    class Dataset:
        def __init__(self, a):
            self.a, self.RasterXSize, self.RasterYSize = a, a.shape[1], a.shape[0]

        def GetRasterBand(self, _i):
            return Band(self.a)

        def FlushCache(self):
            pass

    captured = {}
    gdal = types.SimpleNamespace()
    gdal.TranslateOptions = lambda srcWin=None, format=None: srcWin
    gdal.Translate = lambda path, ds, options=None: Dataset(ds.a[options[1]:options[1] + options[3], options[0]:options[0] + options[2]].copy())
    gdal.GDT_Byte = 1

    class Driver:
        def Create(self, path, xs, ys, bands, kind):
            ds = Dataset(np.zeros((ys, xs), np.uint8))
            band = Band(ds.a)
            band.WriteArray = lambda arr: None
            ds.GetRasterBand = lambda _i: band
            return ds
    gdal.GetDriverByName = lambda _n: Driver()
    cv2 = types.SimpleNamespace(CV_8U=0)
    cv2.imwrite = lambda path, arr: captured.__setitem__(path, np.array(arr))
    cv2.Laplacian = lambda img, ddepth, ksize=1: O.laplacian_u8(img, ksize)
    rcs.gdal, rcs.cv2 = gdal, cv2

    service = rcs.ChipService()
    total = 0
    for name, ref, mon, x0, y0, dx, dy, ksizes in chip_cases():
        out[f"crc_{name}"] = np.array([crc(ref, mon, x0, y0, dx, dy)], np.uint32)
        frame = pd.DataFrame({"x0": x0, "y0": y0, "dx": dx, "dy": dy}).astype(np.float64)
        for ks in ksizes:
            tag = f"{name}_{ktag(ks)}"
            written, names = [], []
            arrays = {"ref_u8": [], "mon_u8": [], "ref_lap": [], "mon_lap": []}
            for i, row in frame.iterrows():                      # (what DataFrame.apply(axis=1) does, one capture per row)
                captured.clear()
                service._to_chips_gdal_dataset(row, monitored=Dataset(mon), reference=Dataset(ref), out_dir=Path("c"), monitored_filename="m",
                                               reference_filename="r", laplacian_ksize=ks, out_dir_laplacian=None if ks is None else Path("l"))
                rn, mn = f"REF_{int(x0[i])}_{int(y0[i])}", f"MON_{int(x0[i])}_{int(y0[i])}"
                names.append(f"{rn} {mn}")
                hit = f"c/r/{rn}.png" in captured
                assert hit == (f"c/m/{mn}.png" in captured) and len(captured) == (0 if not hit else 2 if ks is None else 4)
                written.append(hit)
                if not hit:
                    continue
                arrays["ref_u8"].append(captured[f"c/r/{rn}.png"])
                arrays["mon_u8"].append(captured[f"c/m/{mn}.png"])
                if ks is not None:
                    arrays["ref_lap"].append(captured[f"l/r/{rn}.png"])
                    arrays["mon_lap"].append(captured[f"l/m/{mn}.png"])
            out[f"written_{tag}"] = np.array(written)
            out[f"names_{tag}"] = np.array(names)
            for key, v in arrays.items():
                if v:
                    a = np.stack(v)
                    assert a.dtype == np.uint8 and a.shape[1:] == (57, 57)
                    out[f"{key}_{tag}"] = a
                    total += len(v)
                    if key.endswith("lap"):
                        const = [j for j in range(len(a)) if (a[j] == a[j].flat[0]).all()]
                        u8 = arrays[key.replace("lap", "u8")]
                        assert all((u8[j] == u8[j].flat[0]).all() for j in const), f"{tag}: a Laplacian chip of content is flat"
    path = os.path.join(HERE, "chips.npz")
    np.savez_compressed(path, **out)
    print("chips.npz written:", os.path.getsize(path), "bytes,", total, "chip images")


if __name__ == "__main__":
    main()
