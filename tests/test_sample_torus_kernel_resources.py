"""The sampling kernel of periodic grids, cross-compiled for gfx950 (no GPU needed): csrc/hmg_sample_torus.hip,
k_sample_torus<DIM, RASTER> for 2D / 3D x point list / raster, held to k_sample's limits (tests/test_sample_kernel_resources.py):
no scratch, no spilled register, no LDS, and within 64 vector registers -- eight waves per SIMD, since the kernel hides the
latency of its dependent loads by occupancy alone.  What the compiler reports is the first part of profiles/sample_torus.txt
(`python tests/test_sample_torus_kernel_resources.py` prints it in that form)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
FNAME = "hmg_sample_torus.hip"
NAME = r"\d+(k_sample_torus)ILi(\d+)ELb(\d+)EE"
EXPECTED = {("k_sample_torus", d, r) for d in (2, 3) for r in (0, 1)}
VGPR_LIMIT = 64


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


def report(found):
    lines = [f"csrc/{FNAME} for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage",
             f"{'kernel <DIM, RASTER>':<28}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "LDS", "occupancy", "spills"))]
    for key, v in sorted(found.items()):
        lines.append(f"{key[0] + '<' + ', '.join(str(x) for x in key[1:]) + '>':<28}" +
                     "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                                     "Occupancy [waves/SIMD]")) + f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}")
    return "\n".join(lines)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_torus_sample_kernels_have_no_scratch_no_spills_and_no_lds(tmp_path):
    found = resources(tmp_path)
    assert set(found) == EXPECTED, sorted(found)
    for inst, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (inst, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (inst, v)
        assert v["LDS Size [bytes/block]"] == 0, (inst, v)
        assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT, (inst, v)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        print(report(resources(d)))
