"""Batched units under geometric priors, without a GPU: the facts that keep tests/test_gpu_units_prior.py from being
vacuous (oracle and restatement alone: these two tests say nothing about the library and pass without the feature), the call
`submit_units(priors=)` makes against a recording stand-in of the library, the host half of a batch's frames against `match_tile(prior=)`'s, and a stand-alone g++ -fsanitize=address,undefined program that walks
km_klt_units_frame_prior_submit on the stand-in HIP layer (tests/hoststub/units_prior_main.cpp).

The program runs its refusals and its pipelined prior / plain / prior submissions with the happens-before checker of stub_order.hpp
on and requires that it reports nothing (and, as a control, that it does report two unordered writes).  What the checker cannot see
there: the batched mask launcher's host form writes the units' masks with plain loops and declares nothing, and the seeded prepare /
launch are the unseeded stand-ins, so the seeds behind the lane's table are not declared - the order of those two is argued in
DESIGN.md and held on the GPU by the test of alternating submissions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lk_prior_restatement as PR
import test_resident_calls_host as H0
import units_prior_cases as UC
from karios_amd import _lib, frames
from karios_amd import resident as R
from karios_amd.matcher import prior as prior_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")


# ---------------------------------------------------------------------------- the cases
def test_cases_are_what_the_gpu_tests_need(O):
    units = UC.units()
    assert len({tuple(u["prior"]) for u in units}) >= 2 and all((u["box"] or (0, 0, 700, 560))[2] >= 512 for u in units)
    assert any(u["box"] is not None and u["box"][2] % 2 == 1 for u in units) and any(u["origin"] is not None for u in units)
    for which in "AB":
        ref, mon = UC.pair(which, 7, 3)
        assert ref.min() >= 1 and mon.min() >= 1 and np.array_equal(mon[3:, 7:], ref[:-3, :-7])
        r16, _ = UC.pair(which, 7, 3, dtype="uint16")
        assert r16.dtype == np.uint16 and np.array_equal(r16, ref.astype(np.uint16) * 257)
    n_corners = []
    for k, u in enumerate(units):
        rb, mb, x_off, y_off = UC.unit_boxes(u)
        m = PR.mask(rb, mb, u["prior"], x_off=x_off, y_off=y_off)
        lr = O.laplacian_u8(O.to_uint8(rb), UC.KSIZE)
        p0 = O.good_features(lr, m, UC.MAX_CORNERS_RESTATED, 0.1, 1, 3)
        n_corners.append(0 if p0 is None else len(p0))
        if k == UC.LARGE_SHIFT_UNIT:
            # the prior's mask differs from the base (all valid: no pixel is 0) along two rims, and corners are lost there
            assert m[:30].sum() == 0 and m[:, -40:].sum() == 0 and m[30:, :-40].all()
            free = O.good_features(lr, np.ones_like(m), UC.MAX_CORNERS_RESTATED, 0.1, 1, 3)
            assert {tuple(p) for p in free.reshape(-1, 2)} != {tuple(p) for p in p0.reshape(-1, 2)}
    assert all(n >= 20 for n in n_corners), n_corners


def test_every_unit_keeps_rows_and_the_round_trip_cut_drops_some(O):
    """The restatement's tracker on every unit at the corner count of the unit held to it (60: plain numpy): every unit has >= 20
    corners and >= 5 rows that survive the forward-backward cut, and in at least one unit the cut drops rows."""
    facts = []
    for u in UC.units():
        rb, mb, x_off, y_off = UC.unit_boxes(u)
        m = PR.mask(rb, mb, u["prior"], x_off=x_off, y_off=y_off)
        lr, lm = O.laplacian_u8(O.to_uint8(rb), UC.KSIZE), O.laplacian_u8(O.to_uint8(mb), UC.KSIZE)
        p0 = O.good_features(lr, m, UC.MAX_CORNERS_RESTATED, 0.1, 1, 3)
        g, ok = PR.guess(u["prior"], p0, x_off, y_off)
        assert ok.all(), u["name"]
        p1, p0r = PR.track_fb(lr, lm, p0, g, UC.WIN)
        facts.append((len(p0), int((PR.fb_columns(p0, p1, p0r)[1] < 0.1).sum())))
    print(facts)
    assert all(20 <= n <= UC.MAX_CORNERS_RESTATED and kept >= 5 for n, kept in facts), facts
    assert any(kept < n for n, kept in facts), facts


# ---------------------------------------------------------------------------- submit_units against a recording library
class Lib(H0.Lib):
    """... that also keeps the whole table of priors a call carries."""

    def _km_klt_units_frame_prior_submit(self, *a):
        self.tables.append(np.ctypeslib.as_array(a[-2], shape=(a[1] * 9,)).copy())
        a[-1]._obj.value = 9


def _ctx():
    ctx = H0.make_ctx()
    ctx.lib = Lib()
    ctx.lib.tables = []
    return ctx


def _plain_pair(ctx, base=0):
    return R.ResidentPair.from_device_pointers(H0.MON + base, H0.REF + base, np.uint16, H0.H, H0.W, ctx=ctx)


def test_without_priors_the_old_entry_point_and_the_old_transcript():
    ctx = _ctx()
    a = _plain_pair(ctx)
    pend = R.submit_units([(a, H0.BOX, None), (a, None, None)], H0.make_conf(outliers_filtering=True), 0.4)
    calls = ctx.lib.take()
    assert [c[0] for c in calls] == ["km_set_option", "km_klt_units_frame_submit", "km_set_option"] and pend.prior_steps is None
    assert [c[1] for c in calls if c[0] == "km_set_option"] == [(b"frame_clip", 1), (b"frame_clip", 0)]
    assert len(calls[1][1]) == 9 and ctx.lib.tables == []


@pytest.mark.parametrize("clip", (False, True))
def test_with_priors_the_new_entry_point_the_table_in_unit_order_and_the_clip_off(clip):
    ctx = _ctx()
    a, b = _plain_pair(ctx), _plain_pair(ctx, 0x100000)
    units = [(a, H0.BOX, None), (a, None, (3, 5)), (b, (0, 0, 40, 8), None)]
    P = [PR.shift_prior(1, 2), np.arange(9.0).reshape(3, 3) + 1, [1, 0, -4.5, 0, 1, 0.25, 0, 0, 1]]
    pend = R.submit_units(units, H0.make_conf(outliers_filtering=clip), 0.4, mutual_info=True, priors=P)
    calls = ctx.lib.take()
    assert [c[0] for c in calls] == ["km_set_option", "km_klt_units_frame_prior_submit", "km_set_option"]
    assert [c[1] for c in calls if c[0] == "km_set_option"] == [(b"frame_mi", 1), (b"frame_mi", 0)]          # ("frame_clip" stays off)
    arr, n, code, nr, nm, prm, thr, cap, first, ticket = calls[1][1]
    assert (n, code, nr, nm, prm, thr, cap, ticket) == (3, 1, None, None, ("prm", 50, 3, 3, 0), 0.4, 50, -1)
    want = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in P])
    assert first == tuple(want[:9]) and ctx.lib.tables[0].tobytes() == want.tobytes()
    assert [(arr[k].x_off, arr[k].y_off) for k in range(3)] == [(8.0, 4.0), (3.0, 5.0), (0.0, 0.0)]
    assert (pend.ticket, len(pend)) == (9, 3)
    assert [(tuple(s.P), s.x_off, s.y_off, s.clip) for s in pend.prior_steps] == [(tuple(want[9 * k:9 * k + 9]), x, y, clip) for k, (x, y) in
                                                                                  enumerate([(8, 4), (3, 5), (0, 0)])]
    # one prior for all units; the repeat of a flagged unit is the tile call under that unit's prior
    R.submit_units(units, H0.make_conf(), priors=P[2])
    assert ctx.lib.tables[1].tobytes() == np.tile(np.asarray(P[2], np.float64), 3).tobytes()
    ctx.lib.take()
    pend._raws = [None] * 3
    pend.redo(1)
    (name, args), = [c for c in ctx.lib.take() if c[0].startswith("km_klt")]
    assert name == "km_klt_tile_frame_prior_dev" and tuple(want[9:18]) in args and (3.0, 5.0) == args[12:14]


def test_priors_that_do_not_fit_and_refusals():
    ctx = _ctx()
    a = _plain_pair(ctx)
    two = [(a, H0.BOX, None), (a, H0.BOX, None)]
    with pytest.raises(ValueError):
        R.submit_units(two, H0.make_conf(), priors=[PR.shift_prior(1, 2)] * 3)
    with pytest.raises(ValueError):
        R.submit_units(two, H0.make_conf(), priors=[1.0, 0, np.nan, 0, 1, 0, 0, 0, 1])
    # the shape decides: a one-unit list holds one prior per unit, nine values are one prior for all
    from karios_amd.resident.tiles import _unit_priors
    P = PR.shift_prior(1, 2)
    assert [p.shape for p in _unit_priors([P], 1)] == [(9,)] and [p.shape for p in _unit_priors([P.reshape(3, 3)], 1)] == [(9,)]
    assert len(_unit_priors(P.reshape(3, 3), 4)) == 4 and len(_unit_priors([P, P.reshape(3, 3).tolist()], 2)) == 2
    with pytest.raises(ValueError):
        _unit_priors([P], 2)
    assert ctx.lib.take() == []
    ctx.lib.fail["km_klt_units_frame_prior_submit"] = _lib.E_UNSUPPORTED
    assert R.submit_units(two, H0.make_conf(), priors=PR.shift_prior(1, 2)) is None
    ctx.lib.fail["km_klt_units_frame_prior_submit"] = _lib.E_ARG
    with pytest.raises(R.KariosHipError):
        R.submit_units(two, H0.make_conf(), priors=PR.shift_prior(1, 2))


# ---------------------------------------------------------------------------- the host half of a batch's frames
def _block(cap, rows, seed):
    rng = np.random.default_rng(seed)
    blk = np.zeros(frames.block_words(cap, 0), np.float32)
    blk[:4].view(np.int32)[:] = (rows, rows + 3, 0, 0)
    x0 = np.sort(rng.integers(0, 500, rows)).astype(np.float32) + 100
    cols = [x0, rng.integers(0, 300, rows).astype(np.float32) + 50, rng.normal(4.0, 0.4, rows).astype(np.float32),
            rng.normal(-2.0, 0.4, rows).astype(np.float32), rng.random(rows).astype(np.float32)]
    for k, col in enumerate(cols):
        blk[4 + k * cap:4 + k * cap + rows] = col
    blk[4 + 5 * cap:4 + 5 * cap + rows].view(np.int32)[:] = rng.permutation(rows)
    return blk


@pytest.mark.parametrize("clip", (False, True))
def test_a_batchs_frames_take_the_host_steps_of_match_tile_under_a_prior(monkeypatch, clip):
    from karios_amd import ops
    monkeypatch.setattr(ops, "sigma_clip", lambda dx, dy, ctx=None: frames.sigma_clip(dx, dy))
    cap, P = 40, [PR.shift_prior(4.5, -2.25), UC.units()[4]["prior"]]
    origins = [(100.0, 50.0), (0.0, 0.0)]
    raws = [R.RawFrame(_block(cap, 30, 1), cap, 0), R.RawFrame(_block(cap, 25, 2), cap, 0)]
    pend = R.PendingBatch(H0.make_ctx(), 3, cap, 0, [None, None], [R.pending.PriorSteps(p, x, y, clip) for p, (x, y) in zip(P, origins)])
    pend._raws = raws
    for k in range(2):
        want = frames.block_to_frame(raws[k].block.copy(), cap, 0)
        want["dx_prior"], want["dy_prior"] = prior_mod.prior_columns(want, P[k], *origins[k])
        if clip:
            want = prior_mod.clip_residuals(want)
        got = pend.frame(k)
        assert got.equals(want) and list(got.columns[-2:]) == ["dx_prior", "dy_prior"] and len(got) >= 5


# ---------------------------------------------------------------------------- the stand-alone sanitizer program
@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/libkarios_host_asan.so"])
    d = tmp_path_factory.mktemp("units_prior_main")
    exe, masks = d / "units_prior_main", d / "masks.bin"
    objs = sorted(os.path.join(STUB, "_build", f) for f in os.listdir(os.path.join(STUB, "_build")) if f.endswith(".o"))
    flags = "-std=c++17 -O1 -g -fPIC -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer".split()
    subprocess.check_call(["g++", *flags, "-I" + STUB, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", str(exe),
                           os.path.join(STUB, "units_prior_main.cpp"), *objs, "-ldl", "-lpthread"])
    out = subprocess.run([str(exe), str(masks)], capture_output=True, text=True, timeout=600)
    return out, masks.read_bytes() if masks.exists() else b""


def test_the_entry_point_on_the_stand_in_layer_under_the_sanitizers(program_output):
    out, _ = program_output
    assert out.returncode == 0 and "UNITS-PRIOR OK" in out.stdout and not out.stderr, (out.returncode, out.stderr[-4000:])


def test_the_host_form_of_the_batched_mask_equals_the_restatement(program_output):
    _, got = program_output
    h, w = 64, 512
    i = np.arange(h * w, dtype=np.uint64)

    def raster(mul, shift):
        v = (((i * np.uint64(mul)) & np.uint64(0xFFFFFFFFFFFFFFFF)) >> np.uint64(shift)) % np.uint64(9000)
        return np.where(v % np.uint64(17) == 0, 0, v).astype(np.uint16).reshape(h, w)
    ref, mon = raster(2654435761, 20), raster(40503, 7)
    base = np.where((i * np.uint64(7)) % np.uint64(5) != 0, 3, 0).astype(np.uint8).reshape(h, w)
    priors = [[1, 0, 3, 0, 1, -2, 0, 0, 1], [0.9999, -0.01, 5.5, 0.01, 0.9999, 1.25, 0, 0, 1]]
    want = [PR.mask(ref, mon, priors[0], nodata_ref=0.0, nodata_mon=0.0),
            PR.mask(ref[8:56], mon[8:56], priors[1], base=base[8:56], nodata_ref=0.0, nodata_mon=0.0, x_off=100.0, y_off=8.0)]
    assert 0 < want[0].sum() < want[0].size and 0 < want[1].sum() < want[1].size
    assert got == want[0].tobytes() + want[1].tobytes()
