"""The per-cell histogram kernel, cross-compiled for gfx950 (no GPU needed): csrc/hmg_histogram.hip, k_cell_histogram<DIM, NT, VAR>
for 2D / 3D x 64, 256, 512 threads x the three ways of bringing counts into LDS (0 one add per element, 1 a node's elements
combined first, 2 and the wave's first bin summed across lanes).  Every instantiation without scratch and without a spilled
register, and within 128 vector registers (VGPRs + AGPRs): four waves per SIMD, the bound of the extrema kernels.  Its LDS is
dynamic (lattice image, histogram, sized by the host), so none is asserted.  What the compiler reports is recorded in
profiles/cell_histogram_kernel_resources.txt (`python tests/test_cell_histogram_kernel_resources.py` rewrites it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
REPORT = os.path.join(ROOT, "profiles", "cell_histogram_kernel_resources.txt")
FNAME = "hmg_histogram.hip"
NAME = r"\d+(k_cell_histogram)ILi(\d+)ELi(\d+)ELi(\d+)EE"
EXPECTED = {("k_cell_histogram", d, nt, var) for d in (2, 3) for nt in (64, 256, 512) for var in (0, 1, 2)}
VGPR_LIMIT = 128


def resources(workdir):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", FNAME)
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        m = re.search(NAME, blk.split()[0])
        if m is None:
            continue
        vals = {}
        for f in FIELDS:
            q = re.search(re.escape(f) + r": (\d+)", blk)
            if q:
                vals[f] = int(q.group(1))
        found[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = vals
    return found


def write_report(found):
    with open(REPORT, "w") as f:
        f.write(f"csrc/{FNAME} for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage (LDS is dynamic: sized by the host)\n")
        f.write(f"{'kernel':<40}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "spills")) + "\n")
        for key, v in sorted(found.items()):
            f.write(f"{key[0] + '<' + ', '.join(str(x) for x in key[1:]) + '>':<40}" +
                    "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")) +
                    f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}\n")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cell_histogram_kernels_have_no_scratch_and_no_spills(tmp_path):
    found = resources(tmp_path)
    assert set(found) == EXPECTED, sorted(found)
    for inst, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (inst, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (inst, v)
        assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT, (inst, v)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_report(resources(d))
    print(open(REPORT).read())
