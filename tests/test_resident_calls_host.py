"""What `karios_amd.resident` hands to the library, call by call (CPU only).

The real `ResidentPair`, `submit_units`, `PendingFrame` and `PendingBatch` run over a stand-in for `ctx.lib` that records
(entry point, argument values) and returns 0; the recorded sequences are compared with transcripts written out here from
`include/karios_hip.h`.  The context is a `Context.__new__` with the fields it needs, so its real `check`, `set_option`, `get_option`,
`set_frame_sink` and `run_or_defer` run; pairs come from `from_device_pointers` with made-up addresses.  No library is loaded and no
device is touched."""
import ctypes as C
import gc
import itertools
import os
import sys
import threading
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from karios_amd import _lib, frames  # noqa: E402
from karios_amd import resident as R  # noqa: E402

HANDLE = 0xC0FFEE
REF, MON, MASK, DEV = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # made-up device addresses
H, W = 24, 40
BOX = (8, 4, 16, 12)                       # x_off, y_off, x_size, y_size
WINDOW = (100, 200, 1000, 2000)            # ox, oy, image y_size, image x_size
NO_REF, NO_MON = 0, 65535


class _Any:
    """An address of host memory the transcript cannot know."""

    def __eq__(self, other):
        return True

    def __repr__(self):
        return "ANY"


ANY = _Any()


def plain(a):
    """A ctypes argument as a value: pointers through `.value`, `byref` arguments through `._obj`."""
    if hasattr(a, "_obj"):
        a = a._obj
    if isinstance(a, _lib.KltParams):
        return ("prm", a.max_corners, a.ksize_mon, a.ksize_ref, a.invert_mon)
    if isinstance(a, C._Pointer):          # the prior's nine values
        return tuple(a[:9])
    if isinstance(a, C._SimpleCData):
        return a.value
    return a                               # numbers, bytes, None, arrays (km_unit[])


class Lib:
    """Stand-in for `ctx.lib`: every entry point records its call and returns 0 (`fail[name]`: that status, once); the few that write
    through a pointer have a handler."""

    def __init__(self):
        self.calls, self.fail, self.kept = [], {}, []
        self.block = None                  # what km_frame_wait points at
        self.points = 2                    # rows km_d2h delivers behind km_klt_tile_dev

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args):
            if name == "km_last_error":
                return b"stand-in"
            if name == "km_stage_name":
                return b"stage%d" % args[0]
            self.calls.append((name, tuple(plain(a) for a in args[1:])))      # (without the context handle)
            rc = self.fail.pop(name, 0)
            if rc:
                return rc
            handler = getattr(type(self), "_" + name, None)
            if handler is not None:
                handler(self, *args[1:])
            return 0
        return call

    def take(self):
        out, self.calls = self.calls, []
        return out

    # ---- handlers
    def _km_dev_alloc(self, nbytes, out):
        self.kept.append(nbytes)
        out._obj.value = DEV + 0x1000000 * len(self.kept)

    def _km_host_alloc(self, nbytes, out):
        self.kept.append((C.c_char * nbytes)())
        out._obj.value = C.addressof(self.kept[-1])

    def _km_upload_mark(self, ticket):
        ticket._obj.value = 5

    def _km_frame_wait(self, ticket, blk, nbytes):
        blk._obj.value, nbytes._obj.value = self.block.ctypes.data, self.block.nbytes

    def _km_frame_stage_ms(self, ticket, buf, cap, n):
        buf[0], buf[1], n._obj.value = 1.5, 2.5, 2

    def _km_get_klt_stats(self, stats):
        stats._obj.valid_pixels = 1

    def _km_d2h(self, dst, src, nbytes):
        if nbytes == 4:
            C.cast(dst, C.POINTER(C.c_int32))[0] = self.points
        else:
            C.memset(dst, 0, nbytes)

    def _header(self, host_out):
        C.memset(host_out, 0, 16)          # {n_rows, n_init, flags, candidates} = 0: no frame

    def _km_klt_tile_frame_dev(self, *a):
        self._header(a[-2])

    _km_klt_tile_frame_zncc_dev = _km_klt_tile_frame_prior_dev = _km_klt_tile_frame_dev

    def _km_klt_auto_ksize_frame_dev(self, *a):
        self._header(a[-4])

    def _km_klt_tile_frame_submit(self, *a):
        a[-1]._obj.value = 7

    _km_klt_units_frame_submit = _km_klt_tile_frame_submit


def make_ctx():
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.handle, ctx.device = Lib(), C.c_void_p(HANDLE), 0
    ctx._owner, ctx._abandoned, ctx._abandoned_lock, ctx._alive = threading.get_ident(), [], threading.Lock(), [True]
    ctx._options, ctx._frame_sink, ctx._pool, ctx._pool_bytes, ctx._kp_staging = {}, (None, 0, 0), {}, 0, None
    return ctx


def make_pair(ctx, full=True, dtype=np.uint16, base=0):
    """`full`: with a mask, both no-data values and a window; else the same rasters without any of these."""
    if not full:
        return R.ResidentPair.from_device_pointers(MON + base, REF + base, dtype, H, W, ctx=ctx)
    pair = R.ResidentPair.from_device_pointers(MON + base, REF + base, dtype, H, W, ctx=ctx, mask_ptr=MASK + base, no_data_mon=NO_MON,
                                               no_data_ref=NO_REF)
    pair.window = WINDOW
    return pair


def make_conf(**kw):
    conf = dict(maxCorners=50, blocksize=3, matching_winsize=25, qualityLevel=0.1, minDistance=1, laplacian_kernel_size=3,
                laplacian_invert_polarity=False, outliers_filtering=False, tile_size=512, xStart=0)
    conf.update(kw)
    return SimpleNamespace(**conf)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("KARIOS_HIP_SPECULATIVE", raising=False)


# ---------------------------------------------------------------------------- transcripts (include/karios_hip.h)
def prefix(pair, box, prm):
    """const void *d_ref, *d_mon, int dtype, H, W, ptrdiff_t stride_ref, stride_mon, const uint8_t *d_mask, ptrdiff_t stride_mask,
    const double *nodata_ref, *nodata_mon, const km_klt_params *prm - the head of every tile entry point."""
    x, y, bx, by = box if box is not None else (0, 0, W, H)
    off, es = y * W + x, pair.dtype.itemsize
    return (pair.ref_ptr + off * es, pair.mon_ptr + off * es, pair.code, by, bx, W, W, pair.mask_ptr + off if pair.mask_ptr else None, W,
            None if pair.no_data_ref is None else float(pair.no_data_ref), None if pair.no_data_mon is None else float(pair.no_data_mon), prm)


def whole(pair):
    """const void *d_ref_full, *d_mon_full, int H_full, W_full, ptrdiff_t stride_ref_full, stride_mon_full."""
    return (pair.ref_ptr, pair.mon_ptr, H, W, W, W)


def capacity(max_corners, box):
    return max_corners if max_corners > 0 else max(1, ((box[2] * box[3]) if box is not None else H * W) // 4)


def scopes(pair, scored, mi, clip, call):
    """The option / window calls around a tile call, in the order they are made and undone."""
    before, after = [], []
    if scored and pair.window is not None:
        before.append(("km_set_image_window", WINDOW))
        after.insert(0, ("km_set_image_window", (0, 0, 0, 0)))
    if scored and mi:
        before.append(("km_set_option", (b"frame_mi", 1)))
        after.insert(0, ("km_set_option", (b"frame_mi", 0)))
    if clip:
        before.append(("km_set_option", (b"frame_clip", 1)))
        after.insert(0, ("km_set_option", (b"frame_clip", 0)))
    return before + [call] + after


def test_addresses_of_the_box():
    pair = make_pair(make_ctx())
    p = prefix(pair, BOX, None)
    assert p[0] == REF + (4 * 40 + 8) * 2 and p[1] == MON + (4 * 40 + 8) * 2 and p[7] == MASK + 4 * 40 + 8 and p[5:7] == (40, 40) and p[8] == 40
    assert capacity(0, BOX) == 48 and capacity(50, BOX) == 50


CASES = list(itertools.product((True, False), (50, 0), (None, 0.4), (False, True), (False, True), (None, (3, 5))))


@pytest.mark.parametrize("full,max_corners,thr,mi,clip,origin", CASES)
def test_frame_calls(full, max_corners, thr, mi, clip, origin):
    """km_klt_tile_frame_dev / km_klt_tile_frame_zncc_dev through `match_tile` and `match_tile_raw`, km_klt_tile_frame_submit through
    `submit_tile`."""
    ctx = make_ctx()
    pair = make_pair(ctx, full)
    conf = make_conf(maxCorners=max_corners, outliers_filtering=clip)
    cap = capacity(max_corners, BOX)
    x_off, y_off = origin if origin is not None else BOX[:2]
    head = prefix(pair, BOX, ("prm", max_corners, 3, 3, 0)) + (float(x_off), float(y_off))
    scored = thr is not None
    if scored:
        call = ("km_klt_tile_frame_zncc_dev", head + whole(pair) + (0.4, ANY, cap))
    else:
        call = ("km_klt_tile_frame_dev", head + (ANY, cap))
    expected = scopes(pair, scored, mi, clip, call)
    assert pair.match_tile(conf, BOX, thr, origin=origin, mutual_info=mi) is None
    assert ctx.lib.take() == expected
    raw = pair.match_tile_raw(conf, BOX, thr, origin=origin, mutual_info=mi)
    assert ctx.lib.take() == expected
    n_scores = 0 if not scored else (3 if mi else 1)
    assert (raw.cap, int(raw.with_zncc), raw.block.size, raw.n_rows, raw.flags) == (cap, n_scores, frames.block_words(cap, n_scores), 0, 0)
    # the submission: the whole-raster pointers only where there are scores
    full_group = whole(pair) if scored else (None, None) + whole(pair)[2:]
    call = ("km_klt_tile_frame_submit", head + full_group + (0.4 if scored else 0.0, cap, -1))
    pend = pair.submit_tile(conf, BOX, thr, origin=origin, mutual_info=mi)
    assert ctx.lib.take() == scopes(pair, True, mi and scored, clip, call)
    assert (pend.ticket, pend.cap, int(pend.with_zncc)) == (7, cap, n_scores)


def test_whole_pair_is_the_default_box_and_its_origin():
    ctx = make_ctx()
    pair = make_pair(ctx, False)
    conf = make_conf()
    pair.match_tile(conf)
    assert ctx.lib.take() == [("km_klt_tile_frame_dev", prefix(pair, None, ("prm", 50, 3, 3, 0)) + (0.0, 0.0, ANY, 50))]
    pair.match_tile(conf, ksizes=(5, 7), invert_mon=True)
    assert ctx.lib.take()[0][1][11] == ("prm", 50, 5, 7, 1)
    with pytest.raises(R.KariosHipError):
        pair.match_tile(conf, (30, 0, 16, 12))
    with pytest.raises(R.KariosHipError):
        pair.match_tile(make_conf(laplacian_kernel_size="auto"))


@pytest.mark.parametrize("full", (True, False))
@pytest.mark.parametrize("max_corners", (50, 0))
def test_track_tile_call(full, max_corners):
    ctx = make_ctx()
    pair = make_pair(ctx, full)
    cap = capacity(max_corners, BOX)
    status, tracks = pair.track_tile(make_conf(maxCorners=max_corners), BOX, 5, 3, True)
    out = DEV + 0x1000000
    assert status == "ok" and [t.shape for t in tracks] == [(2, 1, 2)] * 3
    assert ctx.lib.take() == [
        ("km_dev_alloc", (max(1, (3 * cap * 8 + 16 + (2 << 20) - 1) >> 21) << 21, None)),
        ("km_klt_tile_dev", prefix(pair, BOX, ("prm", max_corners, 5, 3, 1)) + (out, out + cap * 8, out + 2 * cap * 8, cap, out + 3 * cap * 8)),
        ("km_get_klt_stats", (ANY,)),
        ("km_d2h", (ANY, out + 3 * cap * 8, 4)),
        ("km_d2h", (ANY, out, 16)), ("km_d2h", (ANY, out + cap * 8, 16)), ("km_d2h", (ANY, out + 2 * cap * 8, 16))]
    # results that stay on the device
    assert pair.track_tile(make_conf(maxCorners=max_corners), BOX, out_ptrs=(1, 2, 3, 4, cap)) == ("ok", 2)
    assert ctx.lib.take()[0] == ("km_klt_tile_dev", prefix(pair, BOX, ("prm", max_corners, 3, 3, 0)) + (1, 2, 3, cap, 4))
    with pytest.raises(R.KariosHipError):
        pair.track_tile(make_conf(maxCorners=max_corners), BOX, out_ptrs=(1, 2, 3, 4, cap - 1))
    ctx.lib.points = 0
    assert pair.track_tile(make_conf(maxCorners=max_corners), BOX) == ("no_features", None)


@pytest.mark.parametrize("max_corners,thr,mi,clip,origin", [(50, None, False, False, None), (0, 0.4, False, True, (3, 5)), (50, 0.4, True, False, None),
                                                           (0, None, True, True, (3, 5))])
def test_prior_call(max_corners, thr, mi, clip, origin):
    """Under a prior the whole-raster group is always there, the threshold is 2.0 without one, "frame_clip" stays off."""
    ctx = make_ctx()
    pair = make_pair(ctx)
    prior = [1, 0, 2.5, 0, 1, -1.5, 0, 0, 1]
    with pytest.raises(R.KariosHipError):
        pair.match_tile(make_conf(), BOX, prior=prior)                 # (a windowed pair)
    pair.window = None
    ctx.lib.take()
    conf = make_conf(maxCorners=max_corners, outliers_filtering=clip)
    cap = capacity(max_corners, BOX)
    x_off, y_off = origin if origin is not None else BOX[:2]
    assert pair.match_tile(conf, BOX, thr, origin=origin, mutual_info=mi, prior=prior) is None
    call = ("km_klt_tile_frame_prior_dev", prefix(pair, BOX, ("prm", max_corners, 3, 3, 0)) + (float(x_off), float(y_off)) + whole(pair)
            + (2.0 if thr is None else 0.4, tuple(float(v) for v in prior), ANY, cap))
    assert ctx.lib.take() == scopes(pair, thr is not None, mi, False, call)


@pytest.mark.parametrize("full,max_corners,origin", [(True, 50, None), (False, 0, (3, 5))])
def test_auto_ksize_call(full, max_corners, origin):
    ctx = make_ctx()
    pair = make_pair(ctx, full)
    x_off, y_off = origin if origin is not None else BOX[:2]
    frame, scores, best, n_init = pair.match_tile_auto_ksize(make_conf(maxCorners=max_corners), BOX, invert_mon=True, candidates=(1, 3), origin=origin)
    assert frame is None and sorted(scores) == [(1, 1), (1, 3), (3, 1), (3, 3)] and best == (0, 0) and n_init == 0
    assert ctx.lib.take() == [("km_klt_auto_ksize_frame_dev", prefix(pair, BOX, ("prm", max_corners, 1, 1, 1))
                               + (ANY, 2, float(x_off), float(y_off), ANY, capacity(max_corners, BOX), ANY, ANY))]
    with pytest.raises(R.KariosHipError):
        pair.match_tile_auto_ksize(make_conf(outliers_filtering=True), BOX)


@pytest.mark.parametrize("entry,name", [("match_tile", "km_klt_tile_frame_zncc_dev"), ("submit_tile", "km_klt_tile_frame_submit")])
def test_scopes_are_restored_after_a_call_that_raises(entry, name):
    ctx = make_ctx()
    pair = make_pair(ctx)
    ctx.lib.fail[name] = -1
    with pytest.raises(R.KariosHipError):
        getattr(pair, entry)(make_conf(outliers_filtering=True), BOX, 0.4, mutual_info=True)
    calls = ctx.lib.take()
    assert [c[0] for c in calls] == ["km_set_image_window", "km_set_option", "km_set_option", name, "km_set_option", "km_set_option", "km_set_image_window"]
    assert calls[4:] == [("km_set_option", (b"frame_clip", 0)), ("km_set_option", (b"frame_mi", 0)), ("km_set_image_window", (0, 0, 0, 0))]
    assert ctx.get_option("frame_clip") == 0 and ctx.get_option("frame_mi") == 0


@pytest.mark.parametrize("entry", ("match_tile", "submit_tile"))
def test_a_set_call_that_fails_resets_only_what_was_set_before_it(entry):
    ctx = make_ctx()
    pair = make_pair(ctx)
    conf = make_conf(outliers_filtering=True)
    ctx.lib.fail["km_set_image_window"] = -1
    with pytest.raises(R.KariosHipError):
        getattr(pair, entry)(conf, BOX, 0.4, mutual_info=True)
    assert ctx.lib.take() == [("km_set_image_window", WINDOW)]
    for mi, option in ((True, b"frame_mi"), (False, b"frame_clip")):
        ctx.lib.fail["km_set_option"] = -1
        with pytest.raises(R.KariosHipError):
            getattr(pair, entry)(conf, BOX, 0.4, mutual_info=mi)
        assert ctx.lib.take() == [("km_set_image_window", WINDOW), ("km_set_option", (option, 1)), ("km_set_image_window", (0, 0, 0, 0))]
        assert ctx.get_option("frame_clip") == 0 and ctx.get_option("frame_mi") == 0


def test_clip_of_too_many_rows_is_refused_by_the_raw_forms():
    ctx = make_ctx()
    pair = R.ResidentPair.from_device_pointers(MON, REF, np.uint8, 512, 512, ctx=ctx)
    conf = make_conf(maxCorners=0, outliers_filtering=True)
    assert pair._frame_capacity(conf, None) == 65536 and pair._frame_capacity(conf, BOX) == 48 and pair._frame_capacity(make_conf(), None) == 50
    for entry in (pair.match_tile_raw, pair.submit_tile):
        with pytest.raises(R.KariosHipError):
            entry(conf)
        with pytest.raises(R.KariosHipError):
            entry(make_conf(laplacian_invert_polarity="auto"))
    assert ctx.lib.take() == []


# ---------------------------------------------------------------------------- submit_units
def test_submit_units_fills_the_units():
    ctx = make_ctx()
    a, b = make_pair(ctx), make_pair(ctx, base=0x100000)
    units = [(a, BOX, None), (a, None, (3, 5)), (b, (0, 0, 40, 8), None)]
    pend = R.submit_units(units, make_conf(outliers_filtering=True), 0.4, mutual_info=True)
    calls = ctx.lib.take()
    assert [c[0] for c in calls] == ["km_set_option", "km_set_option", "km_klt_units_frame_submit", "km_set_option", "km_set_option"]
    assert [c[1] for c in calls if c[0] == "km_set_option"] == [(b"frame_mi", 1), (b"frame_clip", 1), (b"frame_clip", 0), (b"frame_mi", 0)]
    arr, n, code, nr, nm, prm, thr, cap, ticket = calls[2][1]
    assert (n, code, nr, nm, prm, thr, cap, ticket) == (3, 1, float(NO_REF), float(NO_MON), ("prm", 50, 3, 3, 0), 0.4, 50, -1)
    fields = [f for f, _ in _lib.KmUnit._fields_]
    got = [{f: getattr(arr[k], f) for f in fields} for k in range(3)]
    for k, (pair, box, (x_off, y_off)) in enumerate([(a, BOX, (8, 4)), (a, (0, 0, W, H), (3, 5)), (b, (0, 0, 40, 8), (0, 0))]):
        off = box[1] * W + box[0]
        assert got[k] == dict(d_ref=pair.ref_ptr + 2 * off, d_mon=pair.mon_ptr + 2 * off, sref=W, smon=W, d_ref_full=pair.ref_ptr,
                              d_mon_full=pair.mon_ptr, sref_f=W, smon_f=W, H=box[3], W=box[2], Hf=H, Wf=W, x_off=float(x_off), y_off=float(y_off),
                              win_ox=100, win_oy=200, win_H=1000, win_W=2000, d_mask=pair.mask_ptr + off, smask=W), k
    assert (pend.ticket, pend.cap, int(pend.with_zncc), len(pend)) == (7, 50, 3, 3)
    # bare units without scores: nothing but the boxes
    p = make_pair(ctx, False)
    pend = R.submit_units([(p, BOX, None), (p, BOX, None)], make_conf())
    (name, (arr, n, code, nr, nm, prm, thr, cap, ticket)), = ctx.lib.take()
    assert (name, n, nr, nm, thr, int(pend.with_zncc)) == ("km_klt_units_frame_submit", 2, None, None, 0.0, 0)
    assert {f: getattr(arr[1], f) for f in fields} == dict(d_ref=REF + 336, d_mon=MON + 336, sref=W, smon=W, d_ref_full=None, d_mon_full=None, sref_f=0,
                                                           smon_f=0, H=12, W=16, Hf=0, Wf=0, x_off=8.0, y_off=4.0, win_ox=0, win_oy=0, win_H=0, win_W=0,
                                                           d_mask=None, smask=0)


def test_submit_units_declines_what_the_batch_form_does_not_cover():
    ctx = make_ctx()
    a = make_pair(ctx, False)
    conf = make_conf()
    two = [(a, BOX, None), (a, BOX, None)]
    assert R.submit_units([], conf) is None and R.submit_units([(a, BOX, None)] * 17, conf) is None
    assert R.submit_units([(a, BOX, None), (make_pair(make_ctx(), False), BOX, None)], conf) is None                      # contexts
    assert R.submit_units([(a, BOX, None), (make_pair(ctx, False, np.uint8), BOX, None)], conf) is None                   # pixel types
    masked = R.ResidentPair.from_device_pointers(MON, REF, np.uint16, H, W, ctx=ctx, mask_ptr=MASK)
    assert R.submit_units([(a, BOX, None), (masked, BOX, None)], conf) is None                                            # masks
    for kw in (dict(no_data_mon=1), dict(no_data_ref=1)):
        other = R.ResidentPair.from_device_pointers(MON, REF, np.uint16, H, W, ctx=ctx, **kw)
        assert R.submit_units([(a, BOX, None), (other, BOX, None)], conf) is None                                         # no-data values
    assert R.submit_units(two, make_conf(maxCorners=0)) is None
    assert R.submit_units(two, make_conf(laplacian_kernel_size="auto")) is None
    assert R.submit_units(two, make_conf(laplacian_invert_polarity="auto")) is None
    assert ctx.lib.take() == []
    ctx.lib.fail["km_klt_units_frame_submit"] = _lib.E_UNSUPPORTED
    assert R.submit_units(two, conf) is None
    ctx.lib.fail["km_klt_units_frame_submit"] = _lib.E_ARG
    with pytest.raises(R.KariosHipError):
        R.submit_units(two, conf)


def _ring(pair):
    return [b for b in getattr(pair, "_raw_ring", None) or [] if b is not None]


@pytest.mark.parametrize("batched", (True, False))
def test_redo_runs_the_exact_path_with_the_sink_off_and_returns_a_private_copy(batched):
    ctx = make_ctx()
    pair = make_pair(ctx, False)
    conf = make_conf()
    ctx.set_option("speculative", 1)
    ctx.set_frame_sink(0x5000, 1024, 64)
    if batched:
        pend = R.submit_units([(pair, None, None), (pair, BOX, (3, 5))], conf, 0.4)
        ctx.lib.block = np.zeros(2 * frames.block_words(50, 1), np.float32)
        pend.wait()
        redo = lambda: pend.redo(1)                                       # noqa: E731
    else:
        pend = pair.submit_tile(conf, BOX, 0.4, origin=(3, 5))
        redo = pend.redo
    ctx.lib.take()
    raw = redo()
    tile = ("km_klt_tile_frame_zncc_dev", prefix(pair, BOX, ("prm", 50, 3, 3, 0)) + (3.0, 5.0) + whole(pair) + (0.4, ANY, 50))
    assert ctx.lib.take() == [("km_set_option", (b"speculative", 0)), ("km_set_frame_sink_pitch", (None, 0, 0)), tile,
                              ("km_set_option", (b"speculative", 1)), ("km_set_frame_sink_pitch", (0x5000, 1024, 64))]
    assert (raw.cap, int(raw.with_zncc), raw.block.size) == (50, 1, frames.block_words(50, 1))
    assert len(_ring(pair)) == 1 and not any(np.shares_memory(raw.block, b) for b in _ring(pair))
    assert (pend.wait()[1] if batched else pend.wait()) is raw
    # a repeat that raises restores both as well
    ctx.lib.fail["km_klt_tile_frame_zncc_dev"] = -1
    with pytest.raises(R.KariosHipError):
        redo()
    assert ctx.lib.take()[-2:] == [("km_set_option", (b"speculative", 1)), ("km_set_frame_sink_pitch", (0x5000, 1024, 64))]
    assert ctx.get_option("speculative") == 1 and ctx.frame_sink == (0x5000, 1024, 64)
    # without a sink it is not touched; the default of "speculative" is 1
    ctx.set_frame_sink(None)
    ctx._options.pop("speculative")
    ctx.lib.take()
    redo()
    assert [c for c in ctx.lib.take() if c[0] != "km_klt_tile_frame_zncc_dev"] == [("km_set_option", (b"speculative", 0)), ("km_set_option", (b"speculative", 1))]


def test_a_frame_without_a_redo_cannot_be_repeated():
    with pytest.raises(R.KariosHipError):
        R.PendingFrame(make_ctx(), 1, 8, 0).redo()


# ---------------------------------------------------------------------------- block ring
def test_match_tile_raw_rotates_three_blocks():
    ctx = make_ctx()
    pair = make_pair(ctx, False)
    conf = make_conf()
    at = [pair.match_tile_raw(conf, BOX, 0.4).block.ctypes.data for _ in range(5)]
    assert len(set(at[:3])) == 3 and at[3] == at[0] and at[4] == at[1]
    assert len(_ring(pair)) == 3 and all(b.size == frames.block_words(50, 3) for b in _ring(pair))


# ---------------------------------------------------------------------------- waiting
def test_pending_frame_wait_copies_the_pinned_block():
    ctx = make_ctx()
    n32 = frames.block_words(8, 1)
    ctx.lib.block = np.arange(n32, dtype=np.float32)
    ctx.lib.block[2] = 0                                                  # (no flags)
    pend = R.PendingFrame(ctx, 3, 8, 1)
    raw = pend.wait()
    assert ctx.lib.take() == [("km_frame_wait", (3, None, 0))]
    assert np.array_equal(raw.block, ctx.lib.block) and not np.shares_memory(raw.block, ctx.lib.block) and (raw.cap, raw.with_zncc) == (8, 1)
    assert pend.wait() is raw and pend.result() is raw and ctx.lib.take() == []
    assert pend.stage_ms() == {"stage0": 1.5, "stage1": 2.5} and ctx.lib.take() == [("km_frame_stage_ms", (3, ANY, 16, 0))]
    ctx.lib.fail["km_frame_wait"] = -3
    with pytest.raises(R.KariosHipError):
        R.PendingFrame(ctx, 4, 8, 1).wait()
    ctx.lib.fail["km_frame_stage_ms"] = -3
    with pytest.raises(R.KariosHipError):
        pend.stage_ms()


def test_pending_batch_wait_slices_the_blocks_and_flushes_on_the_submitting_thread_only():
    ctx = make_ctx()
    n32 = frames.block_words(8, 3)
    ctx.lib.block = np.arange(3 * n32, dtype=np.float32)
    pend = R.PendingBatch(ctx, 9, 8, 3, [None] * 3)
    raws = pend.wait()
    assert ctx.lib.take() == [("km_frame_flush", (9,)), ("km_frame_wait", (9, None, 0))]
    assert len(raws) == len(pend) == 3 and pend.wait() is raws and ctx.lib.take() == []
    for k, raw in enumerate(raws):
        assert np.array_equal(raw.block, ctx.lib.block[k * n32:(k + 1) * n32]) and not np.shares_memory(raw.block, ctx.lib.block)
        assert (raw.cap, raw.with_zncc) == (8, 3)
    assert pend.stage_ms() == {"stage0": 1.5, "stage1": 2.5} and ctx.lib.take() == [("km_frame_stage_ms", (9, ANY, 16, 0))]
    # a worker thread only waits
    other = R.PendingBatch(ctx, 10, 8, 3, [None] * 3)
    got = []
    t = threading.Thread(target=lambda: got.append(other.wait()))
    t.start()
    t.join()
    assert len(got[0]) == 3 and ctx.lib.take() == [("km_frame_wait", (10, None, 0))]
    ctx.lib.fail["km_frame_wait"] = -3
    with pytest.raises(R.KariosHipError):
        R.PendingBatch(ctx, 11, 8, 3, [None]).wait()


# ---------------------------------------------------------------------------- scores
def _columns(n):
    return [np.arange(n, dtype=np.float64) + 10 * k for k in range(4)]


def _staged(ctx, n, n_outputs):
    """(address of the outputs, address of the key-point columns, the columns as staged)."""
    raw = ctx.__dict__["_kp_staging"]
    o = raw.ctypes.data
    f = o + n_outputs * n * 8
    return o, f, raw[n_outputs * n * 8:n_outputs * n * 8 + 16 * n].view(np.float32)


@pytest.mark.parametrize("n", (0, 1, 3))
@pytest.mark.parametrize("full", (True, False))
def test_zncc_and_mutual_info_stage_the_columns(full, n):
    ctx = make_ctx()
    pair = make_pair(ctx, full)
    z = pair.zncc(*_columns(n))
    assert z.shape == (n,) and z.dtype == np.float64
    calls = [c for c in ctx.lib.take() if c[0] != "km_host_alloc"]
    if n == 0:
        assert calls == [] and ctx.__dict__["_kp_staging"] is None
        assert [v.shape for v in pair.mutual_info(*_columns(0))] == [(0,), (0,)] and ctx.lib.take() == []
        return
    o, f, kp = _staged(ctx, n, 1)
    call = ("km_zncc_batch_dev", whole(pair)[:2] + (pair.code, H, W, H, W, W, W, f, f + 4 * n, f + 8 * n, f + 12 * n, n, o))
    window = full
    assert calls == ([("km_set_image_window", WINDOW)] if window else []) + [call] + ([("km_set_image_window", (0, 0, 0, 0))] if window else []) \
        + [("km_ctx_sync", ())]
    assert np.array_equal(kp, np.concatenate(_columns(n)).astype(np.float32))
    st, nmi = pair.mutual_info(*_columns(n))
    o, f, kp = _staged(ctx, n, 2)
    call = ("km_mi_batch_dev", whole(pair)[:2] + (pair.code, H, W, H, W, W, W, f, f + 4 * n, f + 8 * n, f + 12 * n, n, o, o + 8 * n))
    calls = [c for c in ctx.lib.take() if c[0] != "km_host_alloc"]
    assert calls == ([("km_set_image_window", WINDOW)] if window else []) + [call] + ([("km_set_image_window", (0, 0, 0, 0))] if window else []) \
        + [("km_ctx_sync", ())]
    assert st.shape == nmi.shape == (n,) and np.array_equal(kp, np.concatenate(_columns(n)).astype(np.float32))
    # the second identical call is answered from the memo ...
    again = pair.mutual_info(*_columns(n))
    assert ctx.lib.take() == [] and np.array_equal(again[0], st, equal_nan=True) and again[0] is not st
    # ... other key points are not
    pair.mutual_info(*[c + 1 for c in _columns(n)])
    assert "km_mi_batch_dev" in [c[0] for c in ctx.lib.take()]


@pytest.mark.parametrize("n", (0, 1, 3))
@pytest.mark.parametrize("surface", (False, True))
def test_zncc_search_stages_the_columns_and_lays_out_its_outputs(n, surface):
    ctx = make_ctx()
    pair = make_pair(ctx, False)
    found = pair.zncc_search(*_columns(n), radius=2, surface=surface)
    assert found.shift.shape == (n, 2) and found.peak.shape == (n,) and found.offset.shape == (n, 2) and found.status.shape == (n,)
    assert (found.surface.shape == (n, 5, 5)) if surface else found.surface is None
    calls = [c for c in ctx.lib.take() if c[0] != "km_host_alloc"]
    if n == 0:
        assert calls == []
        return
    o, f, kp = _staged(ctx, n, 5 + (25 if surface else 0))
    assert calls == [("km_zncc_search_dev", whole(pair)[:2] + (pair.code, H, W, H, W, W, W, f, f + 4 * n, f + 8 * n, f + 12 * n, n, 2,
                                                                o + 24 * n, o, o + 8 * n, o + 32 * n, o + 40 * n if surface else None)),
                     ("km_ctx_sync", ())]
    assert np.array_equal(kp, np.concatenate(_columns(n)).astype(np.float32))
    windowed = make_pair(ctx)
    with pytest.raises(R.KariosHipError):
        windowed.zncc_search(*_columns(n))


def test_staging_grows_only_and_belongs_to_the_context():
    ctx = make_ctx()
    a, b = make_pair(ctx, False), make_pair(ctx, False)
    a.zncc(*_columns(3))
    first = ctx.__dict__["_kp_staging"]
    b.zncc(*_columns(2))
    assert ctx.__dict__["_kp_staging"] is first
    b.zncc(*_columns(64))
    assert ctx.__dict__["_kp_staging"] is not first and ctx.__dict__["_kp_staging"].nbytes >= 64 * 24


# ---------------------------------------------------------------------------- upload ticket
def _upload(ctx):
    img = np.zeros((H, W), np.uint16)
    pair = R.ResidentPair.upload(img, img, ctx=ctx)
    names = [c[0] for c in ctx.lib.take()]
    assert names == ["km_dev_alloc", "km_dev_alloc", "km_upload_async", "km_upload_async", "km_upload_mark"]
    return pair


def test_upload_ticket_is_joined_once_by_the_first_call():
    ctx = make_ctx()
    pair = _upload(ctx)
    pair._ready()
    assert ctx.lib.take() == [("km_upload_join", (5,))]
    assert not any(b.upload_in_flight for b in pair._owned)
    pair._ready()
    pair._box(None)
    assert ctx.lib.take() == []
    del pair
    gc.collect()
    assert "km_upload_join" not in [c[0] for c in ctx.lib.take()]


def test_unused_upload_ticket_is_given_back_by_the_finalizer():
    ctx = make_ctx()
    pair = _upload(ctx)
    del pair
    gc.collect()
    calls = ctx.lib.take()
    assert calls[0] == ("km_upload_join", (5,)) and [c[0] for c in calls].count("km_upload_join") == 1
    assert [c[0] for c in calls].count("km_upload_wait") == 2             # (the two buffers' uploads were never joined)


def test_finalizer_on_a_foreign_thread_leaves_the_ticket_to_the_owner():
    ctx = make_ctx()
    held = [_upload(ctx)]
    t = threading.Thread(target=lambda: (held.clear(), gc.collect()))
    t.start()
    t.join()
    assert ctx.lib.take() == [] and len(ctx._abandoned) == 3              # the ticket and the two buffers
    ctx.drain()
    calls = ctx.lib.take()
    assert ("km_upload_join", (5,)) in calls and [c[0] for c in calls].count("km_upload_join") == 1


# ---------------------------------------------------------------------------- public surface
NAMES = ["ResidentPair", "DeviceBuffer", "RawFrame", "PendingFrame", "PendingBatch", "submit_units", "shared_pair", "keep_shared_across",
         "invalidate_raster", "forget_shared_pairs", "ZNCC_SEARCH_COLUMNS", "search_columns", "KariosHipError", "_lib"]
ATTRIBUTES = ["_ready", "_box", "_params", "_match_tile_host_clip", "_match_tile_device_frame", "_frame_capacity", "_frame_clip", "window",
              "match_tile", "match_tile_raw", "submit_tile", "track_tile", "match_tile_auto_ksize", "match_pipelined", "match", "zncc", "zncc_search",
              "mutual_info", "score_frame", "chips", "display_ranges", "point_rasters", "phase_offset", "shifted_monitored", "upload",
              "from_windows", "from_device_pointers"]


def test_import_surface():
    for name in NAMES:
        assert hasattr(R, name), name
    assert R._lib is _lib and R.KariosHipError is _lib.KariosHipError
    pair = make_pair(make_ctx())
    for name in ATTRIBUTES:
        assert hasattr(pair, name), name
    assert R.ZNCC_SEARCH_COLUMNS == ["zncc_dx", "zncc_dy", "zncc_peak", "zncc_off_x", "zncc_off_y", "zncc_status"]
    prm = R.ResidentPair._params(make_conf(), (5, 7), True)
    assert (prm.max_corners, prm.ksize_mon, prm.ksize_ref, prm.invert_mon) == (50, 5, 7, 1)
    assert set(R.__all__) <= set(NAMES) and len(set(R.__all__)) == len(R.__all__)
    with pair._frame_clip(True):
        assert pair.ctx.get_option("frame_clip") == 1
    assert pair.ctx.get_option("frame_clip") == 0
    with pair._frame_clip(False):
        pass
    assert [c[1] for c in pair.ctx.lib.take()] == [(b"frame_clip", 1), (b"frame_clip", 0)]


def test_all_lists_the_public_names():
    """`__all__` is the import surface, whole."""
    assert sorted(R.__all__) == sorted(NAMES)


def test_shared_pair_uploads_is_read_through_the_package(monkeypatch):
    monkeypatch.setattr(R.ResidentPair, "upload", classmethod(lambda cls, mon, ref, ctx=None, **kw: object()))
    R.forget_shared_pairs()
    before = R.shared_pair_uploads
    mon, ref = np.zeros((4, 4), np.uint8), np.ones((4, 4), np.uint8)
    first = R.shared_pair(mon, ref, ctx=object())
    assert R.shared_pair_uploads == before + 1
    R.forget_shared_pairs()
    assert first is not None and mon.flags.writeable
