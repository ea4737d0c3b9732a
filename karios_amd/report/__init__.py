"""Mirror of `karios.report`: the key-point chips of a matched pair, selected and cut on the GPU; the display ranges of the overview
figure (`overview`), the mean profiles of the row / column / altitude figures (`commons`), the key-point rasters of the products
(`product_generator`), the altitude column and box statistics of the DEM figures (`shift_by_alt`) and the numbers of the circular-error
figure (`circular_error`) on resident data."""
from .chip_service import CenterAndQuarterCellPointSelector, Chips, ChipService  # noqa: F401
