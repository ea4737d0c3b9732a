"""Mirror of `karios.report`: the key-point chips of a matched pair, selected and cut on the GPU; the display ranges of the overview
figure (`overview`) and the mean profiles of the row / column / altitude figures (`commons`) on resident data."""
from .chip_service import CenterAndQuarterCellPointSelector, Chips, ChipService  # noqa: F401
