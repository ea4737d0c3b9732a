"""numpy-facing wrappers over the C ABI, one per third-party call on the KARIOS hot path.

Names and argument meaning follow the calls the reference makes (cv2.Laplacian, cv2.goodFeaturesToTrack, cv2.calcOpticalFlowPyrLK,
skimage phase_cross_correlation, karios.core.image.shift_image); file:line citations are relative to the reference tree.
All compute happens in libkarios_hip.so on the GPU.

One module per subsystem of the library (its api_*.hip files); `_place` says where a call's arrays live.  Every public name of a module
is a name of this package: callers write `ops.NAME`, and no module here calls another's wrapper, which tests replace by that name.
"""
from __future__ import annotations

from .. import _lib
from .._lib import default_context
from ._place import tensor_np_dtype
from .tile import *
from .score import *
from .align import *
from .prep import *
from .match import *
from .sift import *
from .accuracy import *
from .chips import *
from .report import *
from .mask import *
