"""CPU suite - who releases what a context creates (csrc/common.hpp: the owner types; km_ctx's member order is the release order).

tests/hoststub/lifetime_main.cpp is a program of its own, built from the host objects of the sanitizer build (every api*.hip and
staging.hip, g++ -fsanitize=address,undefined) and the stand-in HIP layer, which counts live streams, events, device and page-locked
allocations.  It takes a context through every lazy creation site, destroys it and requires all four counts to be zero - then again
with every device allocation, page-locked allocation and stream / event creation of a context's life failing in turn.  The sanitizer
runtime is linked into the program: it runs as it is."""
import os
import subprocess

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")


def test_a_context_releases_everything_it_created_also_after_failures():
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/lifetime"])
    out = subprocess.run([os.path.join(STUB, "_build", "lifetime")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CTX-LIFETIME OK" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-6000:]
