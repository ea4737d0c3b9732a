"""CPU suite, part 3 - sanitizers (GPU AddressSanitizer is not available on this pool, so: CPU builds only).

1. The library's HOST half - every csrc/api*.hip (argument validation, workspace slots, upload tickets, frame ring, the host algebra
   and list protocols of the align step) and csrc/staging.hip (the page-locked staging ring and landing arena) - compiled with
   g++ -fsanitize=address,undefined against a stand-in HIP layer (tests/hoststub/: device memory = host memory, kernels = stand-ins;
   those of RANSAC and SIFT are the shared headers ransac_math.hpp / sift_math.hpp) and driven through the product's ctypes
   signatures: driver.py walks the bookkeeping and proves by execution that no asynchronous runtime copy ever touches pageable
   memory, driver_align.py runs the align step's entry points, RANSAC and SIFT bit for bit against their restatements.
2. The CPU oracle (oracle/*.c) under the same sanitizers, running its own known-answer tests.

All run in subprocesses with libasan preloaded into an ordinary python (tests/sanitizer_harness.py).
"""
import os
import re
import subprocess
import sys

from sanitizer_harness import run, san_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")


def test_host_half_of_the_library_under_asan_ubsan():
    subprocess.check_call(["make", "-s", "-C", STUB])
    driver = [sys.executable, os.path.join(STUB, "driver.py")]
    run(driver, "HOST-ASAN OK", 900, san_env(KARIOS_HIP_RING_CHUNK_KB="64", KARIOS_HIP_UPLOAD_CHECKSUM="1"))
    # the default ring geometry (4 x 4 MB) as well
    run(driver, "HOST-ASAN OK", 900, san_env(KARIOS_HIP_RING_CHUNK_KB="4096"), clean_stderr=False)


def test_align_entry_points_under_asan_ubsan():
    """api_align / api_prep / api_match / api_ransac / api_sift.hip: RANSAC and SIFT end to end on the CPU, bit for bit against the
    restatements, the repeat paths and the capacity protocol of SIFT included (tests/hoststub/driver_align.py)."""
    subprocess.check_call(["make", "-s", "-C", STUB])
    run([sys.executable, os.path.join(STUB, "driver_align.py")], "HOST-ASAN ALIGN OK", 600, san_env())


def test_host_build_covers_every_api_file():
    """The HOST list of tests/hoststub/Makefile is every api*.hip of csrc/ plus staging: a new API file joins the sanitizer build (add
    it to HOST, and stand-ins of its launchers to tests/hoststub/stub_kernels*.cpp) instead of silently staying outside it."""
    host = re.search(r"^HOST\s*=\s*(.*)$", open(os.path.join(STUB, "Makefile")).read(), re.M).group(1).split()
    csrc = os.path.join(ROOT, "karios_amd", "csrc")
    want = [f[:-4] for f in os.listdir(csrc) if f.startswith("api") and f.endswith(".hip")] + ["staging"]
    assert sorted(host) == sorted(want), f"tests/hoststub/Makefile HOST = {sorted(host)}, csrc/ holds {sorted(want)}"


def test_the_sanitizer_build_really_reports():
    """Negative control: a read-back larger than the caller's buffer must abort with an AddressSanitizer report."""
    subprocess.check_call(["make", "-s", "-C", STUB])
    code = f"""
import ctypes as C, numpy as np, sys
lib = C.CDLL({os.path.join(STUB, "_build", "libkarios_host_asan.so")!r})
lib.km_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.km_dev_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
lib.km_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
ctx, d = C.c_void_p(), C.c_void_p()
assert lib.km_ctx_create(0, C.byref(ctx)) == 0 and lib.km_dev_alloc(ctx, 4096, C.byref(d)) == 0
small = np.zeros(100, np.uint8)
lib.km_d2h(ctx, small.ctypes.data_as(C.c_void_p), d, 4096)
print("not detected")
"""
    out = subprocess.run([sys.executable, "-c", code], env=san_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "AddressSanitizer" in out.stderr and "not detected" not in out.stdout, out.stderr[-3000:]


def test_oracle_known_answer_tests_under_asan_ubsan():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"])
    env = san_env(KARIOS_ORACLE_SO=os.path.join(ROOT, "oracle", "libkarios_oracle_asan.so"), KARIOS_ORACLE_THREADS="2")
    # the oracle's own known-answer / golden-vector tests (everything in test_oracle_golden.py that is not the slow config-1 pipeline)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_oracle_golden.py"), "-x", "-q", "-p", "no:cacheprovider",
                          "-k", "not config1 and not full"], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr and "runtime error" not in out.stdout, out.stderr[-6000:]
