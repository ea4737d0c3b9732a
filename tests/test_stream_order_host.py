"""CPU suite - stream order: which kernel may read which buffer is decided by the record / wait statements of csrc/api*.hip and staging.hip,
and the stand-in HIP layer executes everything at once - a missing wait changes nothing there, and on the GPU only when the timing falls
that way.

tests/hoststub/order_main.cpp is a program of its own, built from the host objects of the sanitizer build (every api*.hip and staging.hip,
g++ -fsanitize=address,undefined) and the stand-in HIP layer with its happens-before checker switched on (tests/hoststub/stub_order.hpp:
vector clocks per stream, event and host; last writer, readers and accumulators per byte interval of every device allocation; the stand-in
launchers declare what the real launchers read and write).  It runs the model's own controls, then scenarios through the C ABI on fresh
contexts - uploads joined before a pipelined first call, a pipelined submission behind tiles in flight and behind a kernel that writes the
raster, the steady state, the tile path, the next pair's upload - which must end without a report, then each scenario again with every one of
its hipStreamWaitEvent calls ignored in turn: the checker must notice, or the wait is listed in the program with what covers it.  The
sanitizer runtime is linked into the program: it runs as it is."""
import os
import subprocess

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")


def test_streams_are_ordered_wherever_they_share_a_buffer_and_every_wait_is_seen():
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/order"])
    out = subprocess.run([os.path.join(STUB, "_build", "order")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "STREAM-ORDER OK" in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-6000:]
