"""The per-cell moment kernels, cross-compiled for gfx950 (no GPU needed), every instantiation without scratch and without a
spilled register:
  csrc/hmg_fields.hip         k_cell_pair_moments<DIM, NT, SAME>: 2D / 3D x 64, 256, 512 threads x one column or two.  Vector
                              registers and occupancy no worse than the figures of the two separate kernels this one replaced
                              (LDS_BOUNDS): the single-vector form costs what the single-vector kernel did.
  csrc/hmg_fields_window.hip  k_cell_pair_moments_slab<SAME> (3D) and k_cell_pair_moments_rows<SAME> (2D), cells larger than the
                              LDS.  The 2D kernel keeps to 64 vector registers, two 1024-thread workgroups per compute unit as
                              k_apply_rows; the 3D kernel to 128, one workgroup per compute unit.
Their LDS is dynamic (class table, lattice image or rolling window, wave partials, sized by the host), so none is asserted.  What
the compiler reports is recorded in profiles/cell_moments_kernel_resources.txt (`python tests/test_cell_moments_kernel_resources.py`
rewrites it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
REPORT = os.path.join(ROOT, "profiles", "cell_moments_kernel_resources.txt")

# file -> (regex of the mangled kernel names, its groups as a key, the expected keys)
WINDOW_KERNELS = ("k_cell_pair_moments_slab", "k_cell_pair_moments_rows")
FILES = {
    "hmg_fields.hip": (r"\d+(k_cell_pair_moments)ILi(\d+)ELi(\d+)ELb([01])EE",
                       {("k_cell_pair_moments", d, nt, same) for d in (2, 3) for nt in (64, 256, 512) for same in (0, 1)}),
    "hmg_fields_window.hip": (r"\d+(" + "|".join(WINDOW_KERNELS) + r")ILb([01])EE",
                              {(k, same) for k in WINDOW_KERNELS for same in (0, 1)}),
}
VGPR_LIMIT = {"k_cell_pair_moments_slab": 128, "k_cell_pair_moments_rows": 64}
# (DIM, NT, SAME) -> (VGPRs at most, waves per SIMD at least)
LDS_BOUNDS = {(2, 64, 1): (54, 8), (2, 256, 1): (54, 8), (2, 512, 1): (54, 8),
              (3, 64, 1): (92, 5), (3, 256, 1): (94, 5), (3, 512, 1): (94, 5),
              (2, 64, 0): (60, 8), (2, 256, 0): (60, 8), (2, 512, 0): (60, 8),
              (3, 64, 0): (114, 4), (3, 256, 0): (116, 4), (3, 512, 0): (96, 5)}


def resources(workdir, fname):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", fname)
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        m = re.search(FILES[fname][0], blk.split()[0])
        if m is None:
            continue
        vals = {}
        for f in FIELDS:
            q = re.search(re.escape(f) + r": (\d+)", blk)
            if q:
                vals[f] = int(q.group(1))
        found[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = vals
    return found


def write_report(found_by_file):
    with open(REPORT, "w") as f:
        for fname, found in found_by_file.items():
            f.write(f"csrc/{fname} for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage (LDS is dynamic: sized by the host)\n")
            f.write(f"{'kernel':<40}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "spills")) + "\n")
            for key, v in sorted(found.items()):
                args = [str(x) for x in key[1:-1]] + ["true" if key[-1] else "false"]
                f.write(f"{key[0] + '<' + ', '.join(args) + '>':<40}" +
                        "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")) +
                        f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}\n")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("fname", sorted(FILES))
def test_cell_moments_kernels_have_no_scratch_and_no_spills(tmp_path, fname):
    found = resources(tmp_path, fname)
    assert set(found) == FILES[fname][1], sorted(found)
    for inst, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (inst, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (inst, v)
        if inst[0] in VGPR_LIMIT:
            assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT[inst[0]], (inst, v)
        else:
            vgprs, waves = LDS_BOUNDS[inst[1:]]
            assert v["VGPRs"] + v["AGPRs"] <= vgprs and v["Occupancy [waves/SIMD]"] >= waves, (inst, v)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_report({fname: resources(d, fname) for fname in sorted(FILES)})
    print(open(REPORT).read())
