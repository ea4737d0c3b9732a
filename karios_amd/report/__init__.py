"""Mirror of `karios.report`: the key-point chips of a matched pair, selected and cut on the GPU."""
from .chip_service import CenterAndQuarterCellPointSelector, Chips, ChipService  # noqa: F401
