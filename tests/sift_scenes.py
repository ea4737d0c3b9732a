"""Scenes of the SIFT tests, shared by tests/test_gpu_sift.py (the kernels on the GPU) and tests/hoststub/driver_align.py (the
library's host half on the CPU, under the sanitizers).  Nothing here imports the GPU stack."""
import numpy as np

from karios_amd import synth


def scene(kind, h, w):
    if kind == "textured":
        n = max(h, w)
        return np.ascontiguousarray(synth.sift_scene(n, 3 + n)[:h, :w])
    if kind == "flat":
        return np.full((h, w), 117, np.uint8)
    if kind == "binary":                                             # saturated, near-binary: DoG full of ties
        rng = np.random.default_rng(h * 1000 + w)
        coarse = rng.random((h // 4 + 1, w // 4 + 1)) < 0.5
        img = np.kron(coarse, np.ones((4, 4), bool))[:h, :w]
        out = np.where(img, 255, 0).astype(np.uint8)
        out[rng.random((h, w)) < 0.01] = 254
        return out
    if kind == "blob":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.rint(40 + 180 * np.exp(-((yy - h // 2) ** 2 + (xx - w // 2) ** 2) / (2 * 5.0 ** 2))).astype(np.uint8)
    if kind == "lattice":                                            # a dot every 6 pixels: dense extrema, four-fold symmetric patches
        yy, xx = np.mgrid[0:h, 0:w]
        dy, dx = (yy % 6) - 3, (xx % 6) - 3
        return np.rint(60 + 150 * np.exp(-(dy * dy + dx * dx) / 2.0)).astype(np.uint8)
    raise KeyError(kind)
