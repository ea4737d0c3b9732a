"""SIFT of the global align step on the GPU: the object `detect_global_alignment(..., sift=Sift())` takes in place of
cv2.SIFT_create(nfeatures=0, contrastThreshold=0.02, edgeThreshold=10) (reference global_align.py:48-50, 160-166)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .. import ops
from .global_align import SIFT_CONTRAST_THRESHOLD, SIFT_EDGE_THRESHOLD, SIFT_NFEATURES

KeyPoint = namedtuple("KeyPoint", "pt size angle response octave class_id")


class KeyPoints:
    """The key points of one image: a sequence of cv2.KeyPoint-like items (.pt / .size / .angle / .response / .octave) over the
    structured records (`.records`, ops.SIFT_KEYPOINT_DTYPE).  np.asarray(kp) is the float32 [n, 2] array of (x, y), which is
    what `global_align._points` takes; a slice or an index array gives the KeyPoints of those records."""

    def __init__(self, records):
        self.records = records

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            r = self.records[i]
            return KeyPoint((float(r["x"]), float(r["y"])), float(r["size"]), float(r["angle"]), float(r["response"]), int(r["octave"]), -1)
        return KeyPoints(self.records[i])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __array__(self, dtype=None, copy=None):
        pts = np.stack([self.records["x"], self.records["y"]], 1).reshape(-1, 2)
        return pts if dtype is None else pts.astype(dtype)


class Sift:
    """detectAndCompute(image, None) on the GPU (ops.sift_detect_and_compute); nfeatures other than 0 (retainBest) and detection
    masks are not provided."""

    def __init__(self, contrast_threshold: float = SIFT_CONTRAST_THRESHOLD, edge_threshold: float = SIFT_EDGE_THRESHOLD,
                 nfeatures: int = SIFT_NFEATURES, ctx=None):
        if nfeatures != 0:
            raise NotImplementedError(f"Sift: nfeatures = {nfeatures} (only 0, every key point, is provided)")
        self.contrast_threshold = float(contrast_threshold)
        self.edge_threshold = float(edge_threshold)
        self.ctx = ctx

    def detectAndCompute(self, image, mask=None):
        """-> (KeyPoints, float32 descriptors [n, 128]), or (empty KeyPoints, None) when nothing is found, as cv2 does."""
        if mask is not None:
            raise NotImplementedError("Sift.detectAndCompute: detection masks are not provided")
        kp, desc = ops.sift_detect_and_compute(image, contrast_threshold=self.contrast_threshold, edge_threshold=self.edge_threshold,
                                               ctx=self.ctx)
        if isinstance(kp, dict):                                   # device tensors in: the records are small, bring them over
            rec = np.empty(len(desc), ops.SIFT_KEYPOINT_DTYPE)
            for name in ops.SIFT_FIELDS:
                rec[name] = kp[name].cpu().numpy()
            kp, desc = rec, desc.cpu().numpy()
        return KeyPoints(kp), (desc if len(kp) else None)
