"""CPU sanitizer job for the host side of point sampling: tools/sanitize/host_locate.c, a stand-alone program with its own main,
drives hmg_grid_locate (locator build, lattice tables, the evaluation text the kernel shares) on a grid without a context against
the AddressSanitizer + UBSan and the ThreadSanitizer builds of the library (`make asan tsan` in csrc, as tests/test_sanitizers.py
builds them).  No GPU is touched and nothing is preloaded.  Checked: no sanitizer report, and the checksum of everything the call
returned is the same for 1 and 16 setup threads and for every byte AddressSanitizer fills fresh heap memory with."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "homogenization.jl_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "WARNING: ThreadSanitizer", "ThreadSanitizer:")

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None, reason="no ROCm clang / make")]


def _harness(kind, tmp_path):
    subprocess.run(["make", "-C", CSRC, "-j8", kind], check=True, capture_output=True, text=True)
    libdir = os.path.join(CSRC, "build", kind)
    exe = str(tmp_path / f"host_locate_{kind}")
    san = "-fsanitize=address,undefined" if kind == "asan" else "-fsanitize=thread"
    subprocess.run([CLANG, "-std=c99", "-O1", "-g", san, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "sanitize", "host_locate.c"), "-o", exe, "-L" + libdir, "-lhmg_hip", "-lm",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    return exe


def _run(exe, args, **env):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "host_locate: done" in out.stdout, text[-4000:]
    assert not any(b in text for b in BAD), text[-4000:]
    return [l for l in out.stdout.splitlines() if l.startswith("hash ")]


def test_locate_is_clean_under_asan_ubsan_and_does_not_depend_on_heap_contents(tmp_path):
    exe = _harness("asan", tmp_path)
    ref = None
    for threads, fill in (("1", "0"), ("16", "255")):
        got = _run(exe, ["4", "4", "37"], HMG_SETUP_THREADS=threads, UBSAN_OPTIONS="print_stacktrace=1",
                   ASAN_OPTIONS=f"detect_leaks=1:malloc_fill_byte={fill}:max_malloc_fill_size=1073741824")
        assert len(got) == 8
        ref = ref or got
        assert got == ref, (threads, fill)


def test_locate_is_race_free_under_tsan(tmp_path):
    exe = _harness("tsan", tmp_path)
    got = _run(exe, ["4", "3", "37"], HMG_SETUP_THREADS="16", TSAN_OPTIONS="halt_on_error=0")
    assert len(got) == 6
