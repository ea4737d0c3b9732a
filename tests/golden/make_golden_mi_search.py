#!/usr/bin/env python3
"""Generate tests/golden/mi_search.npz by running the REFERENCE's own `_mutual_info` (karios/matcher/mutual_info_service.py:32-63) and
`_mutual_information` (karios/matcher/zncc_service.py:129-151) at every offset of a radius-2 search around 8 key points, on a seeded
120 x 160 uint16 pair and a float32 pair of the same size.

Run where the reference tree is present (see make_golden.py), never on the GPU box:   python tests/golden/make_golden_mi_search.py

The reference has no search of its own: what is pinned are the two VALUES at each offset, on the 57 x 57 chips the reference's
`_extract_chip` cuts (`image[y - 28:y + 29, x - 28:x + 29]`), NaN where the offset's centre fails the bounds rule of
`_compute_mutual_info` (:99-130) or where numpy raises on a non-finite sample (the reference catches that and scores NaN).  The centres
are those of tests/zncc_search_restatement.py; skipped rows hold NaN throughout.  The rows are the first 8 of the shared case list's
(tests/mi_search_cases.py) plus two whose chips hold the float32 pair's non-finite samples.  Only DATA is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402
import mi_search_cases as M  # noqa: E402
import mi_search_restatement as R  # noqa: E402

RADIUS, ROWS = 2, 8
MORE = np.array([(125.0, 30.0, -30.0, 20.0), (60.0, 50.0, -29.0, 22.0)], np.float32)


def main():
    _rklt, rzncc, _rimage, rmi = import_reference()
    out = {"radius": np.int32(RADIUS)}
    for tag, dtype, seed in (("u16", np.uint16, 201), ("f32", np.float32, 202)):
        case = M.Case("golden_" + tag, dtype, RADIUS, ROWS, "texture", seed)
        ref, mon, *cols = (np.ascontiguousarray(a) for a in M.build(case))
        x0, y0, dx, dy = (np.concatenate([c, MORE[:, i]]) for i, c in enumerate(cols))
        n, S = len(x0), 2 * RADIUS + 1
        studholme = np.full((n, S, S), np.nan)
        nmi = np.full((n, S, S), np.nan)
        for k in range(n):
            c = R.centres(x0[k], y0[k], dx[k], dy[k], ref.shape, mon.shape)
            if c is None:
                continue
            X0, Y0, X1, Y1 = c
            chip_ref = ref[Y0 - 28:Y0 + 29, X0 - 28:X0 + 29]
            for oy in range(-RADIUS, RADIUS + 1):
                for ox in range(-RADIUS, RADIUS + 1):
                    x, y = X1 + ox, Y1 + oy
                    if x - 28 < 0 or y - 28 < 0 or x >= mon.shape[1] - 28 or y >= mon.shape[0] - 28:
                        continue
                    chip_mon = mon[y - 28:y + 29, x - 28:x + 29]
                    try:
                        studholme[k, oy + RADIUS, ox + RADIUS] = rmi._mutual_info(chip_ref, chip_mon)
                        nmi[k, oy + RADIUS, ox + RADIUS] = rzncc._mutual_information(chip_ref, chip_mon)
                    except ValueError:
                        pass
        out.update({f"ref_{tag}": ref, f"mon_{tag}": mon, f"cols_{tag}": np.stack([x0, y0, dx, dy]), f"studholme_{tag}": studholme, f"nmi_{tag}": nmi})
        print(tag, "rows with a value:", int((~np.isnan(studholme).all(axis=(1, 2))).sum()), "NaN offsets:", int(np.isnan(studholme).sum()))
    path = os.path.join(HERE, "mi_search.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
