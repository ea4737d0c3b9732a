"""GPU suite - the kernel-size search (km_klt_auto_ksize_frame_dev, csrc/api_auto.hip) in its BATCHED forms, at the smallest shapes that
reach them: W >= 512, H >= 2 * blockSize + 8 and (H + 1) / 2 > winSize (H >= 52 at the default window of 25).  Expected values come
from the reference's loop (klt.py:465-545) carried out with the oracle, never from the library.  Each case runs three times on one
context: the default options (corners as one batch of units, the trackers as one launch), "speculative" 0 (everything one by one) and
"spec_flag" 32 (every unit flagged and repaired through the exact corner path)."""
import itertools

import numpy as np
import pytest

from karios_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(96, 512), (61, 515)]        # the second: an odd height, a width off the 4-pixel grid
KM_PATH_SPEC_RETRY = 16


def _conf():
    from karios_amd.core import KLTConfiguration
    return KLTConfiguration(maxCorners=120, minDistance=6, blocksize=7, laplacian_kernel_size="auto")


_rasters = {}


def _pair(shape):
    if shape not in _rasters:
        _rasters[shape] = synth.make_cross_sensor_pair(shape[0], shape[1], seed=9)[:2]
    return _rasters[shape]


_expected = {}


def _oracle_loop(O, shape, masked, cands):
    """The reference's loop with the oracle, once per case: ratios, the winner, its result ({columns}, Ninit)."""
    key = (shape, masked, tuple(cands))
    if key in _expected:
        return _expected[key]
    conf = _conf()
    mon, ref = _pair(shape)
    if masked:
        mask = np.ones(ref.shape, np.uint8)
        mask[:20, :50] = 0
    else:
        mask, _ = O.auto_mask(mon, ref)
    u8_m, u8_r = O.to_uint8(mon), O.to_uint8(ref)
    laps_m = {k: O.laplacian_u8(u8_m, k) for k in cands}
    laps_r = {k: O.laplacian_u8(u8_r, k) for k in cands}
    p0s = {k: O.good_features(laps_r[k], mask, conf.maxCorners, conf.qualityLevel, conf.minDistance, conf.blocksize) for k in cands}
    want, best, best_ratio, best_res = {}, None, -1.0, None
    for mk, rk in itertools.product(cands, repeat=2):
        res = None if p0s[rk] is None else O.klt_tracker(laps_r[rk], laps_m[mk], mask, conf, p0=p0s[rk])
        if res is None:
            want[(mk, rk)] = 0.0
            continue
        pts, ninit = res
        want[(mk, rk)] = len(pts["x0"]) / ninit if ninit else 0.0
        if want[(mk, rk)] > best_ratio:
            best_ratio, best, best_res = want[(mk, rk)], (mk, rk), res
    _expected[key] = (want, best, best_res)
    return _expected[key]


@pytest.mark.parametrize("masked,cands", [(True, [3, 5, 7]), (True, [7]), (False, [3, 5, 7])], ids=["mask-3x3", "mask-1x1", "automask-3x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=["96x512", "61x515"])
def test_batched_search_matches_oracle_loop_in_every_form(ops, O, shape, masked, cands):
    """Every inlier ratio, the winning pair, Ninit and the winner's five columns bit for bit - all batched, all one by one, and with
    every unit flagged and repaired (path_flags carries KM_PATH_SPEC_RETRY there and only there)."""
    from karios_amd.resident import ResidentPair
    conf = _conf()
    mon, ref = _pair(shape)
    want, best, best_res = _oracle_loop(O, shape, masked, cands)
    if masked:
        mask = np.ones(ref.shape, np.uint8)
        mask[:20, :50] = 0
        pair = ResidentPair.upload(mon, ref, mask)
    else:
        pair = ResidentPair.upload(mon, ref)
    ctx = pair.ctx
    pts = best_res[0]
    order = np.lexsort((pts["y0"], pts["x0"]))
    try:
        for form, (option, value) in {"batched": (None, 0), "one by one": ("speculative", 0), "flagged": ("spec_flag", 32)}.items():
            if option:
                ctx.set_option(option, value)
            frame, scores, got_best, ninit = pair.match_tile_auto_ksize(conf, candidates=cands)
            flags = ctx.stats().path_flags
            ctx.set_option("speculative", 1)
            ctx.set_option("spec_flag", 0)
            print(form, shape, got_best, ninit, scores)
            assert scores == pytest.approx(want, abs=0) and got_best == best and ninit == best_res[1], form
            for col in ("x0", "y0", "dx", "dy", "score"):
                assert np.array_equal(frame[col].to_numpy(), np.asarray(pts[col], np.float32)[order]), (form, col)
            assert bool(flags & KM_PATH_SPEC_RETRY) == (form == "flagged"), (form, flags)
    finally:
        ctx.set_option("speculative", 1)
        ctx.set_option("spec_flag", 0)
