"""The per-cell moment kernels of cells larger than the LDS (csrc/hmg_fields_window.hip), cross-compiled for gfx950 (no GPU
needed): every instantiation -- k_cell_pair_moments_slab (3D) and k_cell_pair_moments_rows (2D), each for two different columns and
for one column given twice -- without scratch and without a spilled register.  Their LDS is dynamic (class table, wave partials
and the rolling window, sized by the host), so none is asserted.  Occupancy: the 2D kernel keeps to 64 vector registers, two
1024-thread workgroups per compute unit as k_apply_rows; the 3D kernel to 128, one workgroup per compute unit.
What the compiler reports is recorded in profiles/cell_moments_window_kernel_resources.txt
(`python tests/test_cell_moments_window_kernel_resources.py` rewrites it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_cell_pair_moments_slab", "k_cell_pair_moments_rows")
INSTANCES = {(k, same) for k in KERNELS for same in (0, 1)}
VGPR_LIMIT = {"k_cell_pair_moments_slab": 128, "k_cell_pair_moments_rows": 64}
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
REPORT = os.path.join(ROOT, "profiles", "cell_moments_window_kernel_resources.txt")


def resources(workdir):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_fields_window.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = blk.split()[0]
        m = re.search(r"\d+(" + "|".join(KERNELS) + r")ILb([01])E", name)
        if m is None:
            continue
        vals = {}
        for f in FIELDS:
            q = re.search(re.escape(f) + r": (\d+)", blk)
            if q:
                vals[f] = int(q.group(1))
        found[(m.group(1), int(m.group(2)))] = vals
    return found


def write_report(found):
    with open(REPORT, "w") as f:
        f.write("csrc/hmg_fields_window.hip for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage (LDS is dynamic: sized by the host)\n")
        f.write(f"{'kernel':<40}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "spills")) + "\n")
        for (k, same), v in sorted(found.items()):
            f.write(f"{k + '<' + ('true' if same else 'false') + '>':<40}" +
                    "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")) +
                    f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}\n")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_window_kernels_have_no_scratch_and_no_spills(tmp_path):
    found = resources(tmp_path)
    assert set(found) == INSTANCES, sorted(found)
    for inst, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (inst, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (inst, v)
        assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT[inst[0]], (inst, v)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_report(resources(d))
    print(open(REPORT).read())
