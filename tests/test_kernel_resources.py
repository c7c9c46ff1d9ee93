"""Register budget of the benchmarked apply instantiations (cross-compiled for gfx950, no GPU needed).  Three 512-thread
workgroups per CU leave 80 VGPRs per lane (MI355X_MICROARCH.md, register table: 6 waves per SIMD); the hot instantiations
must fit without scratch -- one more live value in a shared code path once cost the main fused kernel three spilled
registers without any test noticing (round 3)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# template arguments <DIM, NT, SPT, FUSED, RB, WD, CG, RS, WC, LF> as they appear in the mangled names
BUDGET = {
    # level 6 with the class weights from the cache (WC: what the benchmark runs on a checkerboard)
    "Li3ELi512ELi13ELb0ELi6ELb0ELb0ELb0ELb1ELi0E": (80, 0),     # plain apply / residual
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb1ELi0E": (80, 0),     # fused CG passes, general (batched) load phase
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb1ELi1E": (80, 0),     # ... CG step 0 (one stream, one batch)
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb1ELi2E": (80, 0),     # ... a dead step (two streams, one batch)
    "Li3ELi512ELi13ELb1ELi6ELb0ELb1ELb0ELb1ELi0E": (80, 0),     # residual with the coarse-grid correction staged in the image
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb1ELb1ELi0E": (80, 0),     # local residual with the restriction in its epilogue
    # ... and combined per cell (meshes with more than 1024 distinct coefficient rows, alpha other than +-1)
    "Li3ELi512ELi13ELb0ELi6ELb0ELb0ELb0ELb0ELi0E": (80, 0),
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb0ELb0ELi0E": (80, 0),
    "Li3ELi512ELi13ELb1ELi6ELb0ELb1ELb0ELb0ELi0E": (80, 0),
    "Li3ELi512ELi13ELb1ELi6ELb0ELb0ELb1ELb0ELi0E": (80, 16),
    "Li3ELi256ELi4ELb1ELi4ELb0ELb0ELb0ELb0ELi0E": (80, 0),      # level 5 workgroup kernel (fallback of the one-wave kernel), fused
    "Li3ELi256ELi4ELb1ELi4ELb0ELb0ELb1ELb0ELi0E": (80, 0),      # ... restriction in the epilogue
}
# k_apply_wave<FUSED, CG, RS, SRC> (hmg_apply_wave.hip): one wave per level-5 cell; 16 waves per CU fit the LDS and leave 128
# VGPRs, the instantiations that hold a second set of values across the cell run 12 waves per CU with 168 -- none may spill
# (a spilled table word is reloaded in front of every column load: vmcnt(0) in the middle of the load phase)
WAVE_BUDGET = {
    "Lb0ELb0ELb0ELb0E": (128, 0),     # plain apply
    "Lb0ELb0ELb0ELb1E": (128, 0),     # plain residual
    "Lb1ELb0ELb0ELb0E": (128, 0),     # fused CG passes (4 of the 6 level-5 launches of a V-cycle)
    "Lb1ELb0ELb0ELb1E": (168, 0),     # fused with a source vector
    "Lb1ELb1ELb0ELb1E": (168, 0),     # residual with the coarse-grid correction staged in the image
    "Lb1ELb0ELb1ELb1E": (168, 0),     # local residual with the restriction in its epilogue
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_hot_instantiations_fit_their_register_budget(tmp_path):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: _ZN3hmg7k_applyI(\w+?)EEvNS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)",
                         out.stderr, re.S):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for name, (vgprs, scratch) in BUDGET.items():
        assert name in found, f"instantiation {name} not compiled; have {sorted(found)[:5]} ..."
        assert found[name][0] <= vgprs, (name, found[name])
        assert found[name][1] <= scratch, (name, found[name])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wave_kernel_fits_its_register_budget(tmp_path):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply_wave.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "w.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: _ZN3hmg12k_apply_waveI(\w+?)EEvNS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)",
                         out.stderr, re.S):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for name, (vgprs, scratch) in WAVE_BUDGET.items():
        assert name in found, f"instantiation {name} not compiled; have {sorted(found)}"
        assert found[name][0] <= vgprs, (name, found[name])
        assert found[name][1] <= scratch, (name, found[name])


# hmg_apply_small.hip: k_apply_small<SPT, FUSED> (16 / 20 waves per CU: 128 / 102 VGPRs) and k_apply_pack<FUSED> (level 2, four
# cells per wave, the lane's class row in registers: 16 waves per CU) -- no scratch in any of them
SMALL_BUDGET = {
    "12k_apply_packILb1E": (128, 0),
    "12k_apply_packILb0E": (128, 0),
    "13k_apply_smallILi1ELb1E": (102, 0),
    "13k_apply_smallILi1ELb0E": (102, 0),
    "13k_apply_smallILi3ELb1E": (128, 0),
    "13k_apply_smallILi3ELb0E": (128, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_small_level_kernels_fit_their_register_budget(tmp_path):
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply_small.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "s.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: _ZN3hmg(\w+?)EEvNS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", out.stderr, re.S):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for name, (vgprs, scratch) in SMALL_BUDGET.items():
        assert name in found, f"instantiation {name} not compiled; have {sorted(found)}"
        assert found[name][0] <= vgprs, (name, found[name])
        assert found[name][1] <= scratch, (name, found[name])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_coarse_products_keep_their_row_sums_in_registers(tmp_path):
    """k_coarse_cheb / k_coarse_direction hold the sums of the four rows a 16-lane group works on in a small array.  Picking one of
    them with a loop over the array (instead of a chain of selects) made the backend move the array to LDS -- 8 KB per block, no
    scratch, nothing in the register report -- and the level-1 solve of config 3 went from 0.95 to 3.8 ms (round 4).  LDS of these
    kernels is the few doubles of their block reductions."""
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_kernels.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = 0
    for m in re.finditer(r"Function Name: _ZN3hmg\d+(k_coarse_cheb|k_coarse_direction)E.*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", out.stderr, re.S):
        seen += 1
        assert int(m.group(2)) == 0, m.group(0)[-200:]
        assert int(m.group(3)) <= 128, (m.group(1), m.group(3))
    assert seen == 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_slab2_kernel_fits_one_workgroup_per_cu_without_scratch(tmp_path):
    """hmg_apply_slab.hip: k_apply_slab2<FUSED, NS, SRC, OUT, loader waves, SLOT> (level 7, round 5) -- ONE 1024-thread workgroup per
    CU: 128 VGPRs per lane.  No instantiation may spill: a spilled value of the loaders' ring or of an asm read batch is a scratch
    access in the middle of a stream that must not wait (and the software-pipelined read experiment of the round showed what a
    compiler move of an unwaited asm output does).  Its global stores must be asm statements (csrc/hmg_stencil.hpp st_global): a
    compiler-visible store inside its loops turned every wait into a drain."""
    src = os.path.join(ROOT, "homogenization.jl_amd", "csrc", "hmg_apply_slab.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "s.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: _ZN3hmg\w*?13k_apply_slab2I(\w+?)EEvNS_8LevelDev.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)",
                         out.stderr, re.S):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    # <FUSED, NS, SRC, OUT> with 4 loader waves: 14 combinations, + the restriction form (8 loader waves, SLOT)
    assert len(found) == 15, sorted(found)
    for name, (vgprs, scratch) in found.items():
        assert vgprs <= 128 and scratch == 0, (name, vgprs, scratch)
    text = open(src).read()
    body = text[text.index("k_apply_slab2("):text.index("size_t slab2_lds_bytes")]
    assert "st_global(" in body
    # no plain store through the output / update pointers inside the kernel
    assert not re.search(r"\b(a\.xout|a\.xacc|a\.out|oc|bxo|bxa)\s*\[[^\]]+\]\s*=[^=]", body), "compiler-visible global store in k_apply_slab2"
