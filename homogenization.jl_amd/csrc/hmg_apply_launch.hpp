// What every launcher of an operator-apply kernel does before it launches (hmg_apply.hip, hmg_apply_wave.hip, hmg_apply_small.hip,
// hmg_apply_slab.hip, hmg_apply_rows.hip): count the work items, hand the kernel its own copy of the arguments, and refuse null bases.
#pragma once
#include "hmg_device.hpp"

#include <stdexcept>

namespace hmg {

// work items (cells) of a launch: a cell list, a prefix of the cells, or all of them
inline int64_t apply_work_items(const ApplyArgs &a, const MeshDev &mesh)
{
    return a.cell_list ? a.ncell_list : a.ncells_prefix ? a.ncells_prefix : mesh.ncells;
}

// the kernel's copy of the arguments.  xcd_order (option cell_order): a full-grid launch walks the cells XCD by XCD -- workgroup b
// works on cell_perm[b], XCD x on the x-th eighth of the cells (upload_mesh)
inline ApplyArgs apply_work_args(const Launch &L, const MeshDev &mesh, const ApplyArgs &a, int64_t nwork, bool xcd_order)
{
    ApplyArgs b = a;
    b.nwork = nwork;
    if (xcd_order && L.cell_order && !a.cell_list && !a.ncells_prefix && mesh.cell_perm) {
        b.cell_list = mesh.cell_perm;
        b.ncell_list = nwork;
    }
    return b;
}

// Every device base a kernel dereferences without a test of its own must be there: the kernels guard the OPTIONAL operands
// (out of a fused pass, src, x2, xout, xacc, x3, xcoarse), not these.  (Round 2 lost a GPU box to a store through a null
// base 0x4000 bytes in -- an experimental launch path without this check; a host throw costs nothing.)
// coef: this family reads the cell coefficients (the families that take every weight from the class-weight cache do not)
inline void check_apply_bases(const ApplyArgs &a, const MeshDev &mesh, bool fused, bool coef)
{
    if (!a.x) throw std::runtime_error("operator apply: null input vector");
    if (!fused && !a.out) throw std::runtime_error("operator apply: a plain launch needs an output vector");
    if (fused && (!a.blockpart || !a.scal)) throw std::runtime_error("operator apply: fused launch without its reduction scratch");
    if (coef && !mesh.coef) throw std::runtime_error("operator apply: no operator coefficients on the device (hmg_grid_set_operator)");
    if ((a.flags & 1) && !mesh.dmask) throw std::runtime_error("operator apply: constraint requested without a Dirichlet mask");
}

// families that fold a level transfer into the apply
inline void check_apply_transfers(const ApplyArgs &a)
{
    if (a.xcoarse && !a.xout) throw std::runtime_error("operator apply: folded prolongation without xout");
    if (a.rcoarse && a.ldrc <= 0) throw std::runtime_error("operator apply: epilogue restriction without the coarse column stride");
}

// families whose kernels take the pending x-updates as they come (the others choose an instantiation by them)
inline void check_apply_pending(const ApplyArgs &a, bool fused)
{
    if (fused && (a.xacc || a.x3) && !a.x2) throw std::runtime_error("operator apply: a pending x-update without its direction vector");
    if (fused && a.xacc && a.x3) throw std::runtime_error("operator apply: xacc and x3 exclude each other");
}

// flags bit 7 (x is zero and is not read)
inline void check_apply_zero_input(const ApplyArgs &a, bool fused)
{
    if ((a.flags & 128) && !(fused && a.x3 && a.x2 && a.xout && !a.xcoarse))
        throw std::runtime_error("operator apply: the zero-input form exists for the residual with two pending x-updates only");
}

}  // namespace hmg
