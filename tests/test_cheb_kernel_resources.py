"""The kernels of the Chebyshev-Jacobi smoother (csrc/hmg_cheb.hip) -- the row-sum kernel and the maximum that form its bound, and
its streaming passes --, cross-compiled for gfx950 (no GPU needed): no scratch, no spilled register, no LDS beyond the block
reduction.  They are bound by HBM, not by occupancy, so no VGPR number is asserted; what the compiler reports is recorded in
profiles/cheb_kernel_resources.txt (tools: `python tests/test_cheb_kernel_resources.py` rewrites it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["k_operator_rowabs", "k_cheb_max_fold", "k_cheb_max", "k_cheb_start", "k_cheb_step", "k_cheb_tail"]
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]


def resources(workdir):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_cheb.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.path.join(str(workdir), "f.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = blk.split()[0]
        k = next((k for k in KERNELS if k in name), None)          # (k_cheb_max_fold is listed before its prefix k_cheb_max)
        if k is None:
            continue
        vals = {}
        for f in FIELDS:
            m = re.search(re.escape(f) + r": (\d+)", blk)
            if m:
                vals[f] = int(m.group(1))
        found[name] = (k, vals)
    return found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cheb_kernels_have_no_scratch_and_no_spills(tmp_path):
    found = resources(tmp_path)
    seen = {k for k, _ in found.values()}
    assert seen == set(KERNELS), sorted(seen)
    assert len(found) == 8, sorted(found)                          # rowabs<2>, <3>; tail<0>, <1>; four more
    for name, (k, v) in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] <= 64, (name, v)              # the four wave maxima of block_max


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        found = resources(d)
    path = os.path.join(ROOT, "profiles", "cheb_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("csrc/hmg_cheb.hip for gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage (256-thread blocks)\n")
        f.write(f"{'kernel':<28}" + "".join(f"{c:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "LDS")) + "\n")
        for name, (k, v) in sorted(found.items(), key=lambda kv: (KERNELS.index(kv[1][0]), kv[0])):
            tmpl = re.search(r"ILi(\d)E", name)
            label = k + (f"<{tmpl.group(1)}>" if tmpl else "")
            f.write(f"{label:<28}" + "".join(f"{v[c]:>10}" for c in ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
                                                                    "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")) + "\n")
    print(open(path).read())
