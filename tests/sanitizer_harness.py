"""The one harness of the CPU sanitizer tests (test_host_asan.py, test_ransac_host.py, test_sift_host.py): find gcc's libasan or skip,
build with the sanitizer flags, run a script in a subprocess with libasan preloaded, assert its marker and a clean stderr."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "karios_amd", "csrc")


def san_env(**extra):
    """The environment of a process that loads a sanitizer build into an ordinary python; skips the test where gcc has no libasan."""
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("gcc has no libasan.so")
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="2")
    env.update(extra)
    return env


def build(source, out, shared=True):
    """g++ with -ffp-contract=off under the address and undefined-behaviour sanitizers, against csrc/: a shared object or a program."""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] +
                          (["-shared", "-fPIC"] if shared else []) + ["-Wall", "-Werror", "-I", CSRC, str(source), "-o", str(out)])


def run(argv, marker, timeout, env=None, clean_stderr=True):
    """Run argv under san_env (or `env`): it must exit 0 and print `marker`; no sanitizer may have spoken on stderr."""
    out = subprocess.run(argv, env=env if env is not None else san_env(), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]
    if clean_stderr:
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-6000:]
    return out
