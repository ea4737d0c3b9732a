"""Mirror of `karios.accuracy_analysis`: the statistics of a matched frame, computed on the GPU."""
from .accuracy_statistics import GeometricStat  # noqa: F401
