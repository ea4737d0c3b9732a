#!/usr/bin/env python3
"""Generate tests/golden/zncc_search.npz by running the REFERENCE's own `_zncc2` (karios/matcher/zncc_service.py:45-126) at every
offset of a radius-4 search around 40 key points, on a seeded 128 x 160 uint16 pair and a float32 pair of the same size.

Run where the reference tree is present (see make_golden.py), never on the GPU box:   python tests/golden/make_golden_zncc_search.py

The reference has no search of its own: what is pinned is the VALUE at each offset, `_zncc2(ref, mon, Y0, X0, Y1 + oy, X1 + ox, 21)`,
with its IndexError (a window that leaves the raster) and its zero-variance rule recorded as NaN.  The centres are those of
`ZNCCService._compute_zncc` (:186-238) as tests/zncc_search_restatement.py states them; skipped rows hold NaN throughout.  The rows are the
first 40 of the shared case list's (tests/zncc_search_cases.py): points at all four corners of the admissible range, skipped rows, a
flat template, windows over a flat block, sums at .5, then random rows.  Only DATA is written.

float32 rasters: numpy keeps `_zncc2`'s arithmetic in float32 when it is handed float32 arrays (means, deviations and products round to
24 bits), while the library defines the value on float32 pixels by float64 sums, as its `compute_zncc` path does.  Both are recorded:
`surface_f32` is `_zncc2` on the float64 copies of the same pixels - the reference's formula in the arithmetic the definition names, held
to 1e-9 - and `surface_f32_native` is `_zncc2` on the float32 arrays as they are, which lies 1.4e-7 from it on this content.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402
import zncc_search_cases as Z  # noqa: E402
import zncc_search_restatement as R  # noqa: E402

RADIUS, ROWS = 4, 40


def main():
    _rklt, rzncc, _rimage, _rmi = import_reference()
    out = {"radius": np.int32(RADIUS)}
    for tag, dtype, seed in (("u16", np.uint16, 101), ("f32", np.float32, 102)):
        case = Z.Case("golden_" + tag, dtype, 128, 160, RADIUS, ROWS, "texture", seed)
        ref, mon, x0, y0, dx, dy = (np.ascontiguousarray(a) for a in Z.build(case))
        S = 2 * RADIUS + 1
        surface = np.full((ROWS, S, S), np.nan)
        native = np.full((ROWS, S, S), np.nan)
        ref64, mon64 = ref.astype(np.float64), mon.astype(np.float64)
        for k in range(ROWS):
            c = R.centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape)
            if c is None:
                continue
            X0, Y0, X1, Y1 = c
            for oy in range(-RADIUS, RADIUS + 1):
                for ox in range(-RADIUS, RADIUS + 1):
                    try:
                        if dtype == np.float32:
                            surface[k, oy + RADIUS, ox + RADIUS] = rzncc._zncc2(ref64, mon64, Y0, X0, Y1 + oy, X1 + ox, 21)
                            native[k, oy + RADIUS, ox + RADIUS] = rzncc._zncc2(ref, mon, Y0, X0, Y1 + oy, X1 + ox, 21)
                        else:
                            surface[k, oy + RADIUS, ox + RADIUS] = rzncc._zncc2(ref, mon, Y0, X0, Y1 + oy, X1 + ox, 21)
                    except IndexError:
                        pass
        out.update({f"ref_{tag}": ref, f"mon_{tag}": mon, f"cols_{tag}": np.stack([x0, y0, dx, dy]), f"surface_{tag}": surface})
        if dtype == np.float32:
            out["surface_f32_native"] = native
            print("float32 arithmetic of the reference against its float64 arithmetic:", np.nanmax(np.abs(native - surface)))
        print(tag, "rows with a value:", int((~np.isnan(surface).all(axis=(1, 2))).sum()), "NaN offsets:", int(np.isnan(surface).sum()))
    path = os.path.join(HERE, "zncc_search.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
