"""CPU suite - the host form of an entry point computes what its _dev form computes (csrc/api_score.hip, api_accuracy.hip, api_chips.hip,
api_report.hip; upload_columns of csrc/api.hip).

tests/hoststub/hostforms_main.cpp is a program of its own, built from the host objects of the sanitizer build (every api*.hip and
staging.hip, g++ -fsanitize=address,undefined) and the stand-in HIP layer, where device memory is host memory.  For ZNCC, MI, the
accuracy statistics, the chip selection, the chips, the point rasters, the samples, the mean profiles and the box statistics it calls
the host form and the _dev form on the same data - n in {0, 1, 3, 65}, rasters as windows of wider buffers, null columns where the
interface allows them - and compares the outputs byte for byte; the sanitizers check every copy between caller memory and the
workspace.  The sanitizer runtime is linked into the program: it runs as it is."""
import os
import subprocess

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hoststub")
SECTIONS = ("scores: zncc, mi, dn_keep", "accuracy: statistics", "chips: selection, extraction", "report: mean profiles, box statistics",
            "products: point rasters, samples")


def test_host_forms_compute_what_the_device_forms_compute():
    subprocess.check_call(["make", "-s", "-C", STUB, "_build/hostforms"])
    out = subprocess.run([os.path.join(STUB, "_build", "hostforms")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("HOST-FORMS OK"), out.stdout[-2000:] + out.stderr[-6000:]
    assert out.stderr == "", out.stderr[-6000:]
    assert out.stdout.splitlines()[:-1] == list(SECTIONS), out.stdout[-2000:]
