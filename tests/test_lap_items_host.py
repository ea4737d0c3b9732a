"""CPU suite - the item geometry the Laplacian pass counts valid pixels by and the fused eigenvalue pass reads those counts by
(karios_amd/csrc/lap_items.hpp).

tests/hoststub/lap_items_main.cpp is a program of its own, built here with g++ -fsanitize=address,undefined from the header alone: for
every height 1 .. 200, width 8 .. 700, 8 / 32 / 33 / 160 rows per item and both strip widths it holds the header's count domains to
the kernel's lane rule (shifted last strip included) and to a partition of the image, and the items returned for a rectangle to a
cover of it.  The sanitizer runtime is linked into the program: it runs as it is."""
import os
import subprocess

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")
FLAGS = ["-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror"]


def test_count_domains_partition_the_image_and_rectangles_are_covered():
    build = os.path.join(STUB, "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "lap_items")
    subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, "-o", exe, os.path.join(STUB, "lap_items_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("LAP-ITEMS OK"), out.stdout[-2000:] + out.stderr[-6000:]
    assert out.stderr == "", out.stderr[-6000:]
    assert int(out.stdout.split()[0]) > 10 ** 6        # (the loops ran)


def test_the_kernels_take_their_geometry_from_the_header():
    """The Laplacian kernel states no strip width, shift rule or count origin of its own, and the eigenvalue kernel none of the
    Laplacian pass's: both include lap_items.hpp."""
    csrc = os.path.join(os.path.dirname(STUB), "..", "karios_amd", "csrc")
    lap = open(os.path.join(csrc, "k_lap.hip")).read()
    eig = open(os.path.join(csrc, "k_eig3.hip")).read()
    assert '#include "lap_items.hpp"' in lap and '#include "lap_items.hpp"' in eig
    assert "#define LAPM_VALID_OF" not in lap and "lapi_count_from(" in lap and "lapi_shifted(" in lap and "lapi_row0(" in lap
    assert "lapi_items_of_rect(" in eig and "lapi_area(" in eig and "248" not in eig and "240" not in eig
