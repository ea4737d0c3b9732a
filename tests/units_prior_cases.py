"""Inputs of the tests of batched units under geometric priors (tests/test_units_prior_host.py, tests/test_gpu_units_prior.py).
Everything here is numpy on the CPU; nothing reads the library under test.

The content is built as `lk_prior_cases.canvas` builds it - blocks of 4 px smoothed twice, no pixel 0 - on a canvas large enough for
units of at least 512 columns, which the batch form requires: pair A is 1120 x 620, pair B 700 x 560, each cut twice out of its canvas so
that mon(x + sx, y + sy) == ref(x, y) exactly for an integer shift.  The contrast is full everywhere but in a narrow band along the
raster's rim, so the borders BETWEEN units (the interior of the raster) carry strong corners on both sides."""
from __future__ import annotations

import functools

import numpy as np

from lk_prior_cases import _smooth, rotation_prior

PAD = 48                                   # canvas margin: integer shifts up to 48 px either way
SIZE = {"A": (620, 1120), "B": (560, 700)}     # (H, W)
MAX_CORNERS = 300
MAX_CORNERS_RESTATED = 60                  # the restatement's tracker is plain numpy
KSIZE, WIN = 5, 25


@functools.lru_cache(maxsize=None)
def canvas(which):
    h, w = SIZE[which]
    rng = np.random.default_rng(20261021 + ord(which))
    hh, ww = h + 2 * PAD, w + 2 * PAD
    t = np.kron(rng.integers(0, 256, (hh // 4 + 1, ww // 4 + 1)).astype(np.float64), np.ones((4, 4)))[:hh, :ww]
    t = _smooth(_smooth(t))
    yy, xx = np.mgrid[0:hh, 0:ww]
    r = np.maximum(np.abs(yy - (hh - 1) / 2) / (h / 2), np.abs(xx - (ww - 1) / 2) / (w / 2))      # 0 in the middle, 1 on the rim of `ref`
    env = np.clip(1.0 - (r - 0.9) / 0.08, 0.12, 1.0)
    out = np.clip(np.rint(128 + (t - 128) * env), 1, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pair(which, sx=0, sy=0, dtype="uint8"):
    """-> (ref, mon) of SIZE[which] with mon(x + sx, y + sy) == ref(x, y); uint16: the same content scaled by 257."""
    c = canvas(which)
    h, w = SIZE[which]
    ref = np.ascontiguousarray(c[PAD:PAD + h, PAD:PAD + w])
    mon = np.ascontiguousarray(c[PAD - sy:PAD - sy + h, PAD - sx:PAD - sx + w])
    if dtype == "uint16":
        ref, mon = ref.astype(np.uint16) * 257, mon.astype(np.uint16) * 257
    for a in (ref, mon):
        a.setflags(write=False)
    return ref, mon


def shift_prior(sx, sy):
    return np.array([1.0, 0.0, float(sx), 0.0, 1.0, float(sy), 0.0, 0.0, 1.0])


def units():
    """-> list of dicts: name, which / shift (the pair), box (x, y, w, h) or None, origin or None, prior.  All of one submission."""
    hb, wb = SIZE["B"]
    return [
        dict(name="left box, even shift", which="A", shift=(14, -6), box=(0, 0, 607, 620), origin=None, prior=shift_prior(14, -6)),
        dict(name="right box of odd width, 5 px short of the content", which="A", shift=(14, -6), box=(607, 0, 513, 620), origin=None, prior=shift_prior(9, -2)),
        dict(name="inner box, explicit origin, fractional shift", which="A", shift=(7, 3), box=(300, 50, 640, 512), origin=(5300.0, 7050.0),
             prior=shift_prior(6.6, 3.3)),            # (a shift is the same map at every origin)
        dict(name="odd shift (7, 3)", which="A", shift=(7, 3), box=(0, 0, 560, 620), origin=None, prior=shift_prior(7, 3)),
        dict(name="whole of pair B, rotation 0.3 deg + shift", which="B", shift=(7, 3), box=None, origin=None,
             prior=rotation_prior(0.3, (wb - 1) / 2, (hb - 1) / 2, sx=7.0, sy=3.0)),
        dict(name="large shift (40, -30)", which="A", shift=(40, -30), box=(100, 0, 700, 620), origin=None, prior=shift_prior(40, -30)),
    ]


LARGE_SHIFT_UNIT = 5
RESTATED_UNIT = 3


def unit_boxes(u):
    """-> (ref box, mon box, x_off, y_off) of a unit: the rasters the tile call sees and the origin its key points carry."""
    ref, mon = pair(u["which"], *u["shift"])
    x, y, w, h = u["box"] if u["box"] is not None else (0, 0, ref.shape[1], ref.shape[0])
    x_off, y_off = u["origin"] if u["origin"] is not None else (x, y)
    return ref[y:y + h, x:x + w], mon[y:y + h, x:x + w], float(x_off), float(y_off)
