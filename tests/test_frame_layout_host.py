"""CPU suite - the frame block's one layout, the arena of the kernel-size search and the search in every form (csrc/api_internal.hpp:
km_frame_layout, km_auto_arena_of; csrc/api_auto.hip).

tests/hoststub/frame_main.cpp is a program of its own, built from the host objects of the sanitizer build (every api*.hip and
staging.hip, g++ -fsanitize=address,undefined) and the stand-in HIP layer.  It holds the layout to the words karios_amd.frames reads, the
arena to the formula the search always used, runs km_klt_auto_ksize_frame_dev all batched, with the trackers one by one, all one by one
and with every unit flagged and repaired - the same ratios, winner and frame block in every form - and reads the score columns of a
blocking tile frame and of a three-unit batched submission at the layout's words.  The sanitizer runtime is linked into the program: it
runs as it is."""
import os
import subprocess

from karios_amd import frames

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")


def test_frame_layout_arena_and_every_form_of_the_kernel_size_search():
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/frame"])
    out = subprocess.run([os.path.join(STUB, "_build", "frame")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("FRAME-LAYOUT OK"), out.stdout[-2000:] + out.stderr[-6000:]
    assert out.stderr == "", out.stderr[-6000:]
    # 12 search cases (64 x 512: three candidate counts x three masks; 64 x 40: three masks), the tile frame, the batched submission
    assert sum(line.startswith("search ") for line in out.stdout.splitlines()) == 12, out.stdout[-2000:]
    assert "tile-frame " in out.stdout and "units-frame " in out.stdout, out.stdout[-2000:]


def test_the_program_reads_blocks_at_the_words_of_block_words():
    # frame_main.cpp restates frames.block_words (4 + (6 + 2 k) * cap): held to the Python side here
    for cap in (1, 7, 64, 32768):
        for k in (0, 1, 3):
            assert frames.block_words(cap, k) == 4 + (6 + 2 * k) * cap
