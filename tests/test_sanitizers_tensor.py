"""CPU sanitizer job for the host side of hmg_grid_set_operator_tensor: tools/sanitize/host_tensor.c, a stand-alone program built
against the AddressSanitizer + UBSan + LeakSanitizer build of the library (`make asan` in csrc, as tests/test_sanitizers.py), drives
full tensors per cell through coefficient rows, class table, level-1 assembly, refusals, domain shrink and a partitioned grid with a
NULL context.  No GPU is touched.

Checked: no sanitizer report, the refusals name their cell, and the checksums of the would-be device tables are the same for 1 and
16 setup threads and for both bytes AddressSanitizer fills fresh heap memory with."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "homogenization.jl_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer")

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None, reason="no ROCm clang / make")]


def test_tensor_operator_host_side_is_clean_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CSRC, "-j8", "asan"], check=True, capture_output=True, text=True)
    libdir = os.path.join(CSRC, "build", "asan")
    exe = str(tmp_path / "host_tensor_asan")
    subprocess.run([CLANG, "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "sanitize", "host_tensor.c"), "-o", exe, "-L" + libdir, "-lhmg_hip", "-lm",
                    "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    ref = None
    for threads, fill in (("1", "0"), ("16", "255")):
        env = dict(os.environ, HMG_SETUP_THREADS=threads, UBSAN_OPTIONS="print_stacktrace=1",
                   ASAN_OPTIONS=f"detect_leaks=1:malloc_fill_byte={fill}:max_malloc_fill_size=1073741824")
        out = subprocess.run([exe, "6", "3"], capture_output=True, text=True, timeout=600, env=env)
        text = out.stdout + out.stderr
        assert out.returncode == 0 and "host_tensor: done" in out.stdout, text[-4000:]
        assert not any(b in text for b in BAD), text[-4000:]
        assert "refused: sigma of cell 1295 is not positive definite" in out.stdout
        assert "refused: sigma of cell 1295 is not finite" in out.stdout
        got = [l for l in out.stdout.splitlines() if l.startswith("hash ")]
        assert len(got) == 7
        ref = ref or got
        assert got == ref, (threads, fill)
    assert len(set(l.split()[-1] for l in ref)) == 7        # (every step changed what a device grid would hold)
