"""Register budget of the level-6 first residual that carries three pending x-updates (option "lazy_x"): k_apply<3, 512, 13, FUSED,
6, .., WC, LF = 4> without the restriction epilogue, cross-compiled for gfx950 (no GPU needed).  It runs once per V-cycle over the
whole finest level; like its neighbours (tests/test_kernel_resources.py) it must keep three 512-thread workgroups per CU: at most
80 VGPRs per lane and no scratch.  The compiler's figures are recorded in profiles/lazy_x_kernel_resources.txt."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# template arguments <DIM, NT, SPT, FUSED, RB, WD, CG, RS, WC, LF> as they appear in the mangled names
CARRYING = "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb1ELi4E"
# ... and the two forms it was derived from, which must not have paid for it: the local residual with the same load phase and the
# restriction in its epilogue, and the general fused instantiation the two-update form goes through
NEIGHBOURS = ("Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb1ELb1ELi4E", "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb1ELi0E")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_carrying_residual_keeps_three_workgroups_per_cu(tmp_path):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: _ZN3hmg7k_applyI(\w+?)EEvNS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr, re.S):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    for name in (CARRYING,) + NEIGHBOURS:
        assert name in found, f"instantiation {name} not compiled; have {sorted(found)[:5]} ..."
        vgprs, scratch, waves = found[name]
        print(f"{name}: {vgprs} VGPRs, {scratch} B scratch per lane, {waves} waves per SIMD")
        assert vgprs <= 80 and scratch == 0, (name, found[name])
        assert waves >= 6, (name, found[name])                     # three workgroups of eight waves on four SIMDs
