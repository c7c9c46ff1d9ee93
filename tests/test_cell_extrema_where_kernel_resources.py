"""The located per-cell extrema kernels (hmg_cell_extrema_where), cross-compiled for gfx950 (no GPU needed): in
csrc/hmg_extrema.hip k_cell_extrema_where<DIM, NT> for 2D / 3D x 64, 256, 512 threads, in csrc/hmg_extrema_window.hip
k_extrema_where_slab (3D) and k_extrema_where_rows (2D), 1024 threads each.  None uses scratch or spills a vector register; all
but the slab form spill no scalar register either.  k_extrema_where_slab spills 4 scalar registers (to lanes of a vector register,
no memory): with the codes' address it needs 106 of the 102 scalar registers a wave may hold, where k_cell_extrema_slab sits at
103 -- the bound below is that figure, so that it does not grow unseen.  Vector registers (VGPRs + AGPRs): 128 at most for the 3D
kernels (the slab form runs one workgroup of 16 waves per CU: four waves per SIMD), 64 and no AGPRs for the rows form, which runs
two workgroups per CU as its sibling does; its LDS, the sibling's plus [16][2] ints of codes, stays within 80 KB.
What the compiler reports is recorded in profiles/cell_extrema_where_kernel_resources.txt (`python
tests/test_cell_extrema_where_kernel_resources.py` rewrites it); the kernels of hmg_cell_extrema in the same files are held by
tests/test_cell_extrema_kernel_resources.py and tests/test_cell_extrema_window_kernel_resources.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
CSRC = os.path.join(ROOT, "homogenization.jl_amd", "csrc")
REPORT = os.path.join(ROOT, "profiles", "cell_extrema_where_kernel_resources.txt")
FILES = {"hmg_extrema.hip": r"\d+(k_cell_extrema_where)ILi(\d+)ELi(\d+)EE",
         "hmg_extrema_window.hip": r"\d+(k_extrema_where_slab|k_extrema_where_rows)E"}
EXPECTED = {"hmg_extrema.hip": {("k_cell_extrema_where", d, nt) for d in (2, 3) for nt in (64, 256, 512)},
            "hmg_extrema_window.hip": {("k_extrema_where_slab",), ("k_extrema_where_rows",)}}
VGPR_LIMIT = {"k_cell_extrema_where": 128, "k_extrema_where_slab": 128, "k_extrema_where_rows": 64}
SGPR_SPILL_LIMIT = {"k_cell_extrema_where": 0, "k_extrema_where_slab": 4, "k_extrema_where_rows": 0}
ROWS_LDS_LIMIT = 80 * 1024


def resources(workdir, fname):
    src = os.path.join(CSRC, fname)
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        m = re.search(FILES[fname], blk.split()[0])
        if m is None:
            continue
        vals = {}
        for f in FIELDS:
            q = re.search(re.escape(f) + r": (\d+)", blk)
            if q:
                vals[f] = int(q.group(1))
        found[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = vals
    return found


def constant(fname, name):
    text = open(os.path.join(CSRC, fname)).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


def rows_lds_bytes():
    """LDS of one workgroup of the located rows form: per-wave partials [16][2] doubles, [16][8] ints and [16][2] ints of codes,
    then the window"""
    nt = constant("hmg_cell_window.hpp", "CW_NT")
    assert nt == 1024 and constant("hmg_rows_window.hpp", "RW_NT") == nt
    nw = nt // 64
    return 8 * 2 * nw + 4 * 8 * nw + 4 * 2 * nw + 8 * constant("hmg_rows_window.hpp", "RW_WIN")


def label(key):
    return key[0] + ("<" + ", ".join(str(x) for x in key[1:]) + ">" if len(key) > 1 else "")


def write_report(found):
    with open(REPORT, "w") as f:
        f.write("the located kernels of csrc/hmg_extrema.hip and csrc/hmg_extrema_window.hip for gfx950, hipcc -O3 "
                f"-Rpass-analysis=kernel-resource-usage (LDS is dynamic: sized by the host; rows form: {rows_lds_bytes()} bytes)\n")
        f.write(f"{'kernel':<40}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "spills")) + "\n")
        for key, v in sorted(found.items()):
            f.write(f"{label(key):<40}" +
                    "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")) +
                    f"{v['SGPRs Spill'] + v['VGPRs Spill']:>10}\n")
        f.write("spills: scalar + vector registers.  No kernel uses scratch or spills a vector register.  k_extrema_where_slab misses the\n"
                "target of no spills by 4 SCALAR registers, kept in lanes of a vector register (no memory traffic): the codes' address\n"
                "and the compares' lane masks on top of k_cell_extrema_slab's 103 scalar registers pass the 102 a wave may hold.\n")


def all_resources(workdir):
    found = {}
    for fname in FILES:
        got = resources(workdir, fname)
        assert set(got) == EXPECTED[fname], (fname, sorted(got))
        found.update(got)
    return found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_located_kernels_keep_their_register_budgets(tmp_path):
    found = all_resources(tmp_path)
    for key, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (key, v)
        assert v["VGPRs Spill"] == 0, (key, v)
        assert v["SGPRs Spill"] <= SGPR_SPILL_LIMIT[key[0]], (key, v)
        assert v["VGPRs"] + v["AGPRs"] <= VGPR_LIMIT[key[0]], (key, v)
    assert found[("k_extrema_where_rows",)]["AGPRs"] == 0, found[("k_extrema_where_rows",)]
    assert rows_lds_bytes() <= ROWS_LDS_LIMIT
    # the recorded figures are the compiler's
    recorded = open(REPORT).read()
    for key, v in found.items():
        line = [ln for ln in recorded.splitlines() if ln.startswith(label(key) + " ")]
        assert len(line) == 1, (key, line)
        assert [int(x) for x in line[0][40:].split()] == [v["SGPRs"], v["VGPRs"], v["AGPRs"], v["ScratchSize [bytes/lane]"],
                                                         v["Occupancy [waves/SIMD]"], v["SGPRs Spill"] + v["VGPRs Spill"]], (key, line)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_report(all_resources(d))
    print(open(REPORT).read())
