"""The per-cell histogram kernels of cells larger than the LDS, cross-compiled for gfx950 (no GPU needed):
csrc/hmg_histogram_window.hip holds exactly k_cell_histogram_slab (3D) and k_cell_histogram_rows (2D), 1024 threads each.  Both
without scratch and without a spilled register.  The slab form runs one workgroup per CU (its window takes up to 70 KB, behind it
at most 4 112 B of counters; four waves per SIMD): 128 vector registers (VGPRs + AGPRs).  The rows form runs two workgroups per CU
(eight waves per SIMD): 64 VGPRs, no AGPRs, and at most 80 KB of LDS at the largest histogram (1 027 bins) -- its LDS is dynamic,
[window | counters], sized here from the constants of the sources.  The budgets are derived ones, not what the
compiler happened to give; what it reports is recorded in profiles/cell_histogram_window_kernel_resources.txt (`python
tests/test_cell_histogram_window_kernel_resources.py` rewrites it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
CSRC = os.path.join(ROOT, "homogenization.jl_amd", "csrc")
REPORT = os.path.join(ROOT, "profiles", "cell_histogram_window_kernel_resources.txt")
FNAME = "hmg_histogram_window.hip"
NAME = r"\d+(k_cell_histogram_slab|k_cell_histogram_rows)E"
EXPECTED = {"k_cell_histogram_slab", "k_cell_histogram_rows"}
VGPR_LIMIT = {"k_cell_histogram_slab": 128, "k_cell_histogram_rows": 64}
ROWS_LDS_LIMIT = 80 * 1024
LDS_PER_CU = 160 * 1024


def resources(workdir):
    src = os.path.join(CSRC, FNAME)
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        sym = blk.split()[0]
        m = re.search(NAME, sym)
        if m is None:
            assert "k_" not in sym, sym           # a kernel of this file the test does not know
            continue
        vals = {}
        for f in FIELDS:
            q = re.search(re.escape(f) + r": (\d+)", blk)
            if q:
                vals[f] = int(q.group(1))
        found[m.group(1)] = vals
    return found


def constant(fname, name):
    text = open(os.path.join(CSRC, fname)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


def rows_lds_bytes():
    """LDS of one workgroup of the rows form at the largest histogram: the window, then HIST_MAX_REGULAR + 3 int32 counters
    (an even number of them)."""
    assert constant("hmg_cell_window.hpp", "CW_NT") == 1024 == constant("hmg_rows_window.hpp", "RW_NT")
    nbins = constant("hmg_histogram_device.hpp", "HIST_MAX_REGULAR") + 3
    assert nbins == 1027
    return 8 * constant("hmg_rows_window.hpp", "RW_WIN") + 4 * ((nbins + 1) // 2 * 2)


def write_report(found):
    with open(REPORT, "w") as f:
        f.write(f"csrc/{FNAME} for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage (LDS is dynamic: [window | nbins counters], "
                f"sized by the host for the call's nbins; rows form at 1027 bins: {rows_lds_bytes()} bytes, two workgroups per CU "
                f"{2 * rows_lds_bytes()} of {LDS_PER_CU})\n")
        f.write(f"{'kernel':<40}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "spills")) + "\n")
        for key, v in sorted(found.items()):
            f.write(f"{key:<40}" +
                    "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")) +
                    f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}\n")
        f.write("k_cell_histogram_rows reaches its 64 VGPRs without an occupancy bound and without spills: two workgroups per CU, "
                "as derived.\n")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cell_histogram_window_kernels_keep_their_register_budgets(tmp_path):
    found = resources(tmp_path)
    assert set(found) == EXPECTED, sorted(found)
    for name, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT[name], (name, v)
    assert found["k_cell_histogram_rows"]["AGPRs"] == 0, found["k_cell_histogram_rows"]
    assert rows_lds_bytes() == 9600 * 8 + 4112 <= ROWS_LDS_LIMIT
    assert 2 * rows_lds_bytes() <= LDS_PER_CU


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_report(resources(d))
    print(open(REPORT).read())
