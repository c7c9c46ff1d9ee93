// Grid creation: the kernel tables of hmg_kernel_tables.cpp go to the device -- or, on a host-only grid, into its checksum
// (DryUploads) --, the operator's coefficients and class-weight cache, the partition's cut lists; with the entry points that
// front them (hmg_grid_create*, hmg_grid_set_operator / set_lambda / shrink / set_cut, the hmg_grid_* queries).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace hmg {
namespace {

void upload_mesh(hmg_grid *g)
{
    const MeshTables &M = g->cur();
    const char *xcd_env = std::getenv("HMG_XCD_LISTS");      // (dev knob: 0 = the cut / inner lists as the partition analysis made them)
    const MeshKernelTables K = build_mesh_kernel_tables(M, !(xcd_env && xcd_env[0] == '0'));
    DryUploads dry_scope(!g->ctx, &g->upload_hash);   // host-only grid: the tables are built and checksummed, nothing is uploaded
    hipStream_t s = g->ctx ? g->ctx->stream : nullptr;
    g->d_cells.upload(M.cells, s);
    g->d_face_pairs.upload(M.face_pairs, s);
    g->d_face_partner.upload(K.face_partner, s);
    g->d_edge_ptr.upload(M.edge_ptr, s);
    g->d_edge_ent.upload(M.edge_ent, s);
    g->d_node_ptr.upload(M.node_ptr, s);
    g->d_node_ent.upload(M.node_ent, s);
    g->d_node_first.upload(M.node_first, s);
    g->d_dmask.upload(K.dmask, s);
    g->d_dupmask.upload(M.dupmask, s);
    g->d_mult.upload(M.mult, s);
#ifdef HMG_PHASE_TIMING
    constexpr size_t BP = 10;   // 2 reduction partials + 8 time stamps per workgroup
#else
    constexpr size_t BP = 2;
#endif
    // (+ XS_COUNT: the step length of a pending r-update, its step's beta and the other ratios of pending x-updates live behind the
    //  partials, hmg_grid::pend_alpha())
    if (g->d_blockpart.n < (size_t)M.ncells * BP + XS_COUNT) g->d_blockpart.alloc((size_t)M.ncells * BP + XS_COUNT);
    g->d_cells_cut.upload(K.cells_cut, s);
    g->d_cells_inner.upload(K.cells_inner, s);
    g->d_cell_perm.upload(K.cell_perm, s);
    MeshDev &d = g->md;
    d.dim = M.dim;
    d.ncells = M.ncells;
    d.nnodes = M.nnodes;
    d.cells = g->d_cells.p;
    d.face_pairs = g->d_face_pairs.p;
    d.face_partner = g->d_face_partner.p;
    d.nfacepairs = (int64_t)M.face_pairs.size() / 3;
    d.edge_ptr = g->d_edge_ptr.p;
    d.edge_ent = g->d_edge_ent.p;
    d.nsharededges = (int64_t)M.edge_ptr.size() - 1;
    d.node_ptr = g->d_node_ptr.p;
    d.node_ent = g->d_node_ent.p;
    d.nsharednodes = (int64_t)M.node_ptr.size() - 1;
    d.node_first = g->d_node_first.p;
    d.dmask = g->d_dmask.p;
    d.dupmask = g->d_dupmask.p;
    d.mult = g->d_mult.p;
    d.blockpart = g->d_blockpart.p;
    d.cells_cut = g->d_cells_cut.p;
    d.cells_inner = g->d_cells_inner.p;
    d.ncells_cut = (int64_t)M.cells_cut.size();
    d.ncells_inner = (int64_t)M.cells_inner.size();
    d.cell_perm = g->d_cell_perm.p;          // (XCD x walks the x-th eighth of the cells, see build_mesh_kernel_tables)
    d.ncut_edge_groups = M.ncut_edge_groups;
    d.ncut_node_groups = M.ncut_node_groups;
    d.ncut_face_pairs = M.ncut_face_pairs;
    d.coef = g->d_coef.p;
}

void upload_levels(hmg_grid *g)
{
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    hipStream_t s = g->ctx ? g->ctx->stream : nullptr;
    // LDS of a slab window: half of the CU's, so that two workgroups are resident (HMG_SLAB_LDS_KB overrides, dev knob)
    const char *kb_env = std::getenv("HMG_SLAB_LDS_KB");
    const int slab_kb = kb_env ? std::max(16, std::min(158, std::atoi(kb_env))) : 70;
    g->ld.resize(g->nlevels);
    for (int l = 0; l < g->nlevels; ++l) {
        const LevelTables &T = g->lt[l];
        const LevelTables *C = l > 0 ? &g->lt[l - 1] : nullptr;
        const AddressTables A = build_address_tables(T);
        const BlockedInterior blk = build_blocked_interior(T);
        const SlabWindows sw = build_slab_windows(T, C, slab_kb);
        const TransferTables X = build_transfer_tables(T, C, blk);
        const WaveTables W = build_wave_tables(T, C, blk, X.clpos);
        g->lb.emplace_back(new LevelBufs);
        LevelBufs &B = *g->lb.back();
        // (in this order: a host-only grid's checksum folds in the uploads one after another; an empty table uploads nothing)
        B.meta.upload(T.meta, s);
        B.lpos.upload(A.lpos, s);
        B.pos32.upload(A.pos32, s);
        B.pos32w.upload(A.pos32w, s);
        B.sweep32.upload(A.sweep32, s);
        B.blk_word.upload(blk.word, s);
        B.blk_slot.upload(blk.slot, s);
        B.slab_head.upload(sw.head, s);
        B.slab_ld_word.upload(sw.ld_word, s);
        B.slab_cp_word.upload(sw.cp_word, s);
        B.slab_cp_slot.upload(sw.cp_slot, s);
        B.slab_rs_head.upload(sw.rs_head, s);
        B.slab_rs_word.upload(sw.rs_word, s);
        B.slab_rs_slot.upload(sw.rs_slot, s);
        B.rtab.upload(sw.rtab, s);
        B.sweep_slot.upload(A.sweep_slot, s);
        B.ctab.upload(T.ctab, s);
        B.hier2slot.upload(T.hier2slot, s);
        B.par_a.upload(T.par_a, s);
        B.par32.upload(X.par32, s);
        B.par_b.upload(T.par_b, s);
        B.clpos.upload(X.clpos, s);
        B.par64.upload(X.par64, s);
        B.rs_word.upload(X.rs_word, s);
        B.rs_w.upload(X.rs_w, s);
        B.rs_lp.upload(X.rs_lp, s);
        B.wave_tab.upload(W.tab, s);
        B.wave_lpos.upload(W.lpos, s);
        B.wave_par.upload(W.par, s);
        B.wave_cl.upload(W.cl, s);
        B.wave_rs.upload(W.rs, s);
        B.rptr.upload(T.rptr, s);
        B.ridx.upload(T.ridx, s);
        B.dphi.upload(T.dphi, s);
        B.nslab = sw.nslab;
        B.slab_lds_nodes = sw.lds_nodes;
        B.slab_max_surf = sw.max_surf;
        B.slab_max_int = sw.max_int;
        B.slab_rs_max_surf = sw.rs_max_surf;
        B.slab_rs_max_int = sw.rs_max_int;
        LevelDev &D = g->ld[l];
        D.dim = T.dim;
        D.level = T.level;
        D.m = T.m;
        D.nf = T.nf;
        D.ld = T.ld;
        D.ncorner = T.ncorner;
        D.nedge = T.nedge;
        D.nface = T.nface;
        D.nei = T.nei;
        D.nfi = T.nfi;
        D.nint = T.nint;
        D.off_edge = T.off_edge;
        D.off_face = T.off_face;
        D.off_int = T.off_int;
        D.ncls = T.ncls;
        D.ndir = T.ndir;
        D.nterm = T.nterm;
        D.lds_g0 = T.lds_g0;
        D.lds_g1 = T.lds_g1;
        D.nf_coarse = C ? C->nf : 0;
        D.meta = B.meta.p;
        D.lpos = B.lpos.p;
        D.sweep_slot = B.sweep_slot.p;
        D.pos32 = B.pos32.p;
        D.pos32w = B.pos32w.p;
        D.sweep32 = B.sweep32.p;
        D.nsweep = (int)T.sweep_meta.size();
        D.blk_word = B.blk_word.p;
        D.blk_slot = B.blk_slot.p;
        D.nblk = blk.nblk;
        D.blk_R = blk.R;
        D.ctab = B.ctab.p;
        D.hier2slot = B.hier2slot.p;
        D.par_a = B.par_a.p;
        D.par32 = B.par32.p;
        D.par_b = B.par_b.p;
        D.par64 = B.par64.p;
        D.clpos = B.clpos.p;
        D.rs_word = B.rs_word.p;
        D.rs_w = B.rs_w.p;
        D.rs_lp = B.rs_lp.p;
        D.rptr = B.rptr.p;
        D.ridx = B.ridx.p;
        D.dphi = B.dphi.p;
        D.wave_tab = B.wave_tab.p;
        D.wave_lpos = B.wave_lpos.p;
        D.wave_par = B.wave_par.p;
        D.wave_cl = B.wave_cl.p;
        D.wave_rs = B.wave_rs.p;
        D.wcache = nullptr;                      // (set with the operator: build_weight_cache)
    }
}

// Class-weight cache of the one-wave apply (hmg_apply_wave.hip).  The per-cell weights of the lattice stencil are linear in
// the cell's coefficient row (|J| P_kl, |J|), and on the meshes this library is built for most rows repeat: a checkerboard
// has at most 8 sigma triples x 6 tetrahedron orientations = 48 distinct ones.  Cells are classed by the BITS of their row;
// per class, sign of alpha and level the 15 x 15 weights are formed once on the device (launch_weight_cache), by the same
// products in the same order as the kernels form them per cell.  A field with a row of its own in every cell (one grain
// orientation per cube, a perturbed mesh) is classed like any other: 3 840 B per class and level.  No cache, and the older
// kernels, where the rows outnumber the context's option "weight_cache_classes" (0, the default: no limit by count) or where
// the cache does not fit the device memory (ensure_weight_cache).
void build_cell_classes(hmg_grid *g)
{
    g->nclasses = 0;
    g->wc_ready = false;
    g->md.cell_class = nullptr;
    g->md.nclasses = 0;
    g->cell_class.clear();
    for (auto &d : g->ld) d.wcache = nullptr;
    bool any = false;
    for (const auto &d : g->ld) any = any || d.level >= 2;
    if (!any || g->dim != 3) return;
    const int64_t n = g->cur().ncells;
    const int64_t limit = g->wc_limit;
    struct Key {
        uint64_t b[8];
        bool operator==(const Key &o) const { return std::memcmp(b, o.b, sizeof(b)) == 0; }
    };
    struct Hash {
        size_t operator()(const Key &k) const
        {
            uint64_t h = 1469598103934665603ull;
            for (int q = 0; q < 8; ++q) h = (h ^ k.b[q]) * 1099511628211ull;
            return (size_t)h;
        }
    };
    std::unordered_map<Key, int32_t, Hash> ids;
    std::vector<int32_t> cls((size_t)n);
    std::vector<double> rep;
    for (int64_t c = 0; c < n; ++c) {
        Key k;
        std::memcpy(k.b, g->coef.data() + (size_t)c * 8, sizeof(k.b));
        auto it = ids.find(k);
        if (it == ids.end()) {
            if (limit > 0 && (int64_t)ids.size() >= limit) {          // too many distinct rows: no cache
                release_weight_cache(g);
                return;
            }
            it = ids.emplace(k, (int32_t)ids.size()).first;
            rep.insert(rep.end(), g->coef.begin() + (size_t)c * 8, g->coef.begin() + (size_t)c * 8 + 8);
        }
        cls[(size_t)c] = it->second;
    }
    g->nclasses = (int)ids.size();
    hipStream_t s = g->ctx ? g->ctx->stream : nullptr;
    g->d_cell_class.upload(cls, s);
    g->d_coef_rep.upload(rep, s);
    g->cell_class.swap(cls);
    g->md.cell_class = g->d_cell_class.p;
    g->md.nclasses = g->nclasses;
}

}  // namespace

void release_weight_cache(hmg_grid *g)
{
    bool held = false;
    for (auto &b : g->lb) held = held || (b && b->wcache.p);
    if (held && g->ctx) (void)hipStreamSynchronize(g->ctx->stream);   // (kernels that read the cache)
    for (auto &b : g->lb)
        if (b) b->wcache.release();
    for (auto &d : g->ld) d.wcache = nullptr;
    if (g->ctx) {
        g->ctx->wc_classes -= g->wc_counted_classes;
        g->ctx->wc_bytes -= g->wc_counted_bytes;
    }
    g->wc_counted_classes = g->wc_counted_bytes = 0;
    g->wc_ready = false;
}

// (re)forms the cached weights when the operator or lambda has changed since they were formed; called in front of every
// apply (a host comparison when nothing has changed).  The memory is taken where the operator is set, never in a V-cycle; if
// it is not there the grid keeps the kernels that form their weights per cell, and the context's counters
// "weight_cache_classes" / "weight_cache_bytes" do not count it.
void ensure_weight_cache(hmg_grid *g)
{
    if (!g->md.cell_class || (g->wc_ready && g->wc_lambda == g->lambda)) return;
    const size_t per_level = (size_t)g->nclasses * 2 * WAVE_WSTRIDE;
    int64_t bytes = 0;
    for (int l = 0; l < g->nlevels; ++l) {
        LevelDev &D = g->ld[l];
        if (D.level < 2 || D.ncls != 15) continue;           // (every 3D level an operator is applied on: k_apply<.., WC>, k_apply_wave)
        LevelBufs &B = *g->lb[l];
        if (B.wcache.n < per_level || (g->wc_trim && B.wcache.n != per_level)) {
            HIPCHK(hipStreamSynchronize(g->ctx->stream));   // (kernels that read the old cache)
            B.wcache.release();
            void *q = nullptr;
            if (device_malloc(&q, per_level * sizeof(double)) != hipSuccess) {
                (void)hipGetLastError();
                release_weight_cache(g);
                g->md.cell_class = nullptr;                  // every launcher's eligibility test reads this
                g->cell_class.clear();                       // ... and table "cell_class" reports no classes
                g->ctx->wc_refusals += 1;
                return;
            }
            B.wcache.p = (double *)q;
            B.wcache.n = per_level;
        }
        launch_weight_cache(g->ctx->L, D, g->d_coef_rep.p, g->nclasses, g->lambda, B.wcache.p);
        D.wcache = B.wcache.p;
        bytes += (int64_t)(B.wcache.n * sizeof(double));      // (what is held: after a domain shrink more than the rows in use)
    }
    g->ctx->wc_classes += (int64_t)g->nclasses - g->wc_counted_classes;
    g->ctx->wc_bytes += bytes - g->wc_counted_bytes;
    g->wc_counted_classes = g->nclasses;
    g->wc_counted_bytes = bytes;
    g->wc_lambda = g->lambda;
    g->md.wc_lambda = g->lambda;
    g->wc_ready = true;
    g->wc_trim = false;
}

namespace {

void upload_operator(hmg_grid *g)
{
    const MeshTables &M = g->cur();
    if (g->part) {   // local sigma = rows of the global field
        const int sn = g->sig_n;
        g->sigma.resize((size_t)M.ncells * sn);
        for (int64_t q = 0; q < M.ncells; ++q)
            for (int a = 0; a < sn; ++a)
                g->sigma[(size_t)q * sn + a] = g->sigma_global[(size_t)g->part->cells_g[q] * sn + a];
    }
    build_cell_coefficients(M, g->sigma.data(), g->sig_n, g->coef);
    g->coarse_ready = false;
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    g->d_coef.upload(g->coef, g->ctx ? g->ctx->stream : nullptr);
    g->md.coef = g->d_coef.p;
    build_cell_classes(g);
    if (g->ctx) ensure_weight_cache(g);          // formed here, not in front of the first apply: a V-cycle allocates nothing
}

void set_cut_kind(hmg_grid *g, int k, int64_t nglobal, int64_t n, const int64_t *gid, const int32_t *cell_lid,
                         const int32_t *seg, const int64_t *sidx)
{
    CutKind &c = g->cut[k];
    c.nglobal = nglobal;
    c.nentries = n;
    c.gid.assign(gid, gid + n);
    c.seg.clear();
    c.sidx.clear();
    if (seg && sidx) {
        c.seg.assign(seg, seg + n);
        c.sidx.assign(sidx, sidx + n);
    }
    std::vector<int32_t> hc(cell_lid, cell_lid + n);
    std::vector<uint8_t> first(n, 0);
    std::unordered_map<int64_t, int> seen;
    for (int64_t i = 0; i < n; ++i) {
        need(c.gid[i] >= 0 && c.gid[i] < nglobal, "cut id out of range");
        need((hc[i] >> 3) >= 0 && (hc[i] >> 3) < g->md.ncells, "cut entry references a cell outside the grid");
        if (seen.emplace(c.gid[i], 1).second) first[i] = 1;
    }
    g->cutlv.clear();                            // buffer layouts are rebuilt at the next exchange
    g->cut_agreed_ready = false;                 // ... and the ranks agree on the size of the new cut at the next apply
    g->dinv_ready = false;                       // ... and the smoother's diagonal is summed across the new cut
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    c.cell_lid.upload(hc, g->ctx ? g->ctx->stream : nullptr);
    c.first.upload(first, g->ctx ? g->ctx->stream : nullptr);
}

// device side of the partition tables (after upload_mesh): cut lists, node ownership, global node ids of the cells
void finish_partition(hmg_grid *g)
{
    const Partition &P = *g->part;
    const MeshTables &M = g->cur();
    for (int k = 0; k < 3; ++k)
        set_cut_kind(g, k, P.nglobal[k], (int64_t)P.gid[k].size(), P.gid[k].data(), P.cell_lid[k].data(), P.seg_of[k].data(),
                     P.seg_idx[k].data());
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    hipStream_t s = g->ctx ? g->ctx->stream : nullptr;
    g->d_nodes_g.upload(P.nodes_g, s);
    g->d_owned.upload(P.owned_node, s);
    std::vector<int32_t> cg(M.cells.size());
    for (size_t q = 0; q < cg.size(); ++q) cg[q] = P.nodes_g[M.cells[q]];
    g->d_cells_gnode.upload(cg, s);
}

}  // namespace
}  // namespace hmg

extern "C" {

// part: the grid is this rank's share, by `owner`, of the mesh (cut_owner: rehearsal partitions only, else null)
static int create_grid(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords, int64_t ncells,
                       const int64_t *cells, bool part, const int32_t *owner, const int32_t *cut_owner, int rank, int nranks,
                       hmg_grid **out, const double *period = nullptr)
{
    HMG_TRY
    need(coords && cells && out && (owner || !part), "null argument");
    if (ctx) HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<hmg_grid> g(new hmg_grid);
    g->ctx = ctx;
    g->fuse_cg = ctx ? ctx->fuse_cg_default : true;
    g->dim = dim;
    g->nlevels = nlevels;
    g->lt = build_level_tables(dim, nlevels);
    for (const LevelTables &T : g->lt) g->fields.elem.push_back(build_element_tables(T));   // (host tables: hmg_cell_extrema)
    if (part) {
        g->part.reset(new Partition);
        // The analysis looks at this rank's cells and their one-cell halo (the global pass keeps only what the replicated level-1
        // system needs); HMG_PARTITION_ANALYSIS=global, or HMG_EXCHANGE=allreduce -- which needs cut ids every rank agrees on --,
        // bring back the analysis of the whole mesh on every rank.
        const char *pa = std::getenv("HMG_PARTITION_ANALYSIS"), *ex = std::getenv("HMG_EXCHANGE");
        g->part_halo = !((pa && std::string(pa) == "global") || (ex && std::string(ex) == "allreduce"));
        build_partition(dim, nnodes, coords, ncells, cells, owner, rank, nranks, g->mesh_full, *g->part, cut_owner, g->part_halo);
        g->part_coords.assign(coords, coords + (size_t)dim * nnodes);
        g->part_cells.assign(cells, cells + (size_t)(dim + 1) * ncells);
        g->part_owner.assign(owner, owner + ncells);
        if (cut_owner) g->part_cut_owner.assign(cut_owner, cut_owner + ncells);
        g->part_nnodes = nnodes;
        g->part_ncells = ncells;
    } else if (period) {
        build_mesh_tables_periodic(dim, nnodes, coords, ncells, cells, period, g->mesh_full);
        g->mean_free = true;                     // (no node is constrained: with lambda = 0 the level-1 matrix has the constants in its kernel)
    } else {
        build_mesh_tables(dim, nnodes, coords, ncells, cells, g->mesh_full);
    }
    upload_levels(g.get());
    upload_mesh(g.get());
    if (part) finish_partition(g.get());
    if (ctx) {
        LifetimeLock lock(lifetime_mutex());
        ctx->refs += 1;
    }
    *out = g.release();
    HMG_END
}

int hmg_grid_create(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords, int64_t ncells,
                    const int64_t *cells, hmg_grid **out)
{
    return create_grid(ctx, dim, nlevels, nnodes, coords, ncells, cells, false, nullptr, nullptr, 0, 1, out);
}

int hmg_grid_create_periodic(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords, int64_t ncells,
                             const int64_t *cells, const double *period, hmg_grid **out)
{
    if (!period) {
        last_error() = "hmg_grid_create_periodic: null period";
        return 1;
    }
    return create_grid(ctx, dim, nlevels, nnodes, coords, ncells, cells, false, nullptr, nullptr, 0, 1, out, period);
}

int hmg_grid_create_partition(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords, int64_t ncells,
                              const int64_t *cells, const int32_t *owner, int rank, int nranks, hmg_grid **out)
{
    return create_grid(ctx, dim, nlevels, nnodes, coords, ncells, cells, true, owner, nullptr, rank, nranks, out);
}

int hmg_grid_create_partition_rehearsal(hmg_ctx *ctx, int dim, int nlevels, int64_t nnodes, const double *coords,
                                        int64_t ncells, const int64_t *cells, const int32_t *owner, const int32_t *cut_owner,
                                        int rank, int nranks, hmg_grid **out)
{
    return create_grid(ctx, dim, nlevels, nnodes, coords, ncells, cells, true, owner, cut_owner, rank, nranks, out);
}

// sn numbers per cell (hmg_grid::sig_n) of the whole mesh: the GLOBAL one on a partitioned grid
static void set_operator(hmg_grid *g, const double *sigma, int sn, double lambda)
{
    settle_rebuild(g);                           // (a pending r-update may have its Ap still to form, with the operator it was recorded under)
    if (g->part)
        g->sigma_global.assign(sigma, sigma + (size_t)g->part->global.ncells * sn);
    else
        g->sigma.assign(sigma, sigma + (size_t)g->mesh_full.ncells * sn);
    g->sig_n = sn;
    g->wc_limit = g->ctx ? g->ctx->wc_max_classes : 0;   // read here, and only here: hmg_grid_shrink keeps it
    g->wc_trim = true;
    g->lambda = lambda;
    g->has_op = true;
    g->op_epoch += 1;
    g->dinv_ready = false;
    upload_operator(g);
}

int hmg_grid_set_operator(hmg_grid *g, const double *sigma, double lambda)
{
    HMG_TRY
    need(g && sigma, "null argument");
    set_operator(g, sigma, g->dim, lambda);
    HMG_END
}

int hmg_grid_set_operator_tensor(hmg_grid *g, const double *sigma, double lambda)
{
    HMG_TRY
    need(g && sigma, "null argument");
    const int dim = g->dim, nc = sym_ncomp(dim);
    const int64_t n = g->part ? g->part->global.ncells : g->mesh_full.ncells;
    bool diagonal = true;
    for (int64_t c = 0; c < n; ++c) {   // (nothing of the grid changes before the whole field has passed)
        const double *s = sigma + (size_t)c * nc;
        for (int t = 0; t < nc; ++t)
            if (!std::isfinite(s[t])) throw std::runtime_error("sigma of cell " + std::to_string(c) + " is not finite");
        // positive definite: the leading minors
        bool spd;
        if (dim == 2) {
            spd = s[0] > 0.0 && s[0] * s[2] - s[1] * s[1] > 0.0;
            diagonal = diagonal && s[1] == 0.0;
        } else {
            const double m2 = s[0] * s[3] - s[1] * s[1];
            const double m3 = s[0] * (s[3] * s[5] - s[4] * s[4]) - s[1] * (s[1] * s[5] - s[4] * s[2]) + s[2] * (s[1] * s[4] - s[3] * s[2]);
            spd = s[0] > 0.0 && m2 > 0.0 && m3 > 0.0;
            diagonal = diagonal && s[1] == 0.0 && s[2] == 0.0 && s[4] == 0.0;
        }
        if (!spd) throw std::runtime_error("sigma of cell " + std::to_string(c) + " is not positive definite");
    }
    if (diagonal) {   // the diagonal entry's arithmetic and tables, to the bit
        std::vector<double> d((size_t)n * dim);
        for (int64_t c = 0; c < n; ++c)
            for (int a = 0; a < dim; ++a) d[(size_t)c * dim + a] = sigma[(size_t)c * nc + sym_index(dim, a, a)];
        set_operator(g, d.data(), dim, lambda);
    } else {
        set_operator(g, sigma, nc, lambda);
    }
    HMG_END
}

int hmg_grid_set_lambda(hmg_grid *g, double lambda)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    settle_rebuild(g);                           // (... and with its lambda and class-weight cache)
    g->lambda = lambda;
    g->op_epoch += 1;
    g->dinv_ready = false;
    g->coarse_ready = false;
    if (g->ctx && g->has_op) ensure_weight_cache(g);
    HMG_END
}

int hmg_grid_shrink(hmg_grid *g, int64_t ncells_prefix, int64_t nnodes_prefix)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(!g->mesh_full.periodic(), "hmg_grid_shrink: a periodic grid has no prefix domains (a prefix of a torus is no torus)");
    need(!g->dir_custom, "hmg_grid_shrink: the grid holds a caller's Dirichlet faces (hmg_grid_set_dirichlet_faces); restore the "
                         "default set first (nfaces = -1)");
    if (g->ctx) materialize_r(g);                // (a pending r-update belongs to the cells and face partners of the grid as it is)
    g->op_epoch += 1;
    g->dinv_ready = false;
    g->sample.ready = false;                     // (the locator of hmg_sample.cpp covers the cells as they were)
    if (g->part) {
        // prefix of the GLOBAL mesh: this rank keeps its cells with a global id below the prefix length (local
        // cells are in ascending global order, so that is a prefix of every local level vector as well); cut
        // entities, Dirichlet masks, multiplicities and node ownership are re-derived from the smaller global mesh
        need(ncells_prefix >= 1 && ncells_prefix <= g->part_ncells && nnodes_prefix >= 1 && nnodes_prefix <= g->part_nnodes,
             "prefix out of range");
        const int rank = g->part->rank, nranks = g->part->nranks;
        std::unique_ptr<Partition> np(new Partition);
        MeshTables local;
        build_partition(g->dim, nnodes_prefix, g->part_coords.data(), ncells_prefix, g->part_cells.data(),
                        g->part_owner.data(), rank, nranks, local, *np,
                        g->part_cut_owner.empty() ? nullptr : g->part_cut_owner.data(), g->part_halo);
        need(local.ncells <= g->mesh_full.ncells, "shrunk partition is larger than the original one");
        g->mesh = std::move(local);
        g->part = std::move(np);
        g->shrunk = true;
        upload_mesh(g);
        finish_partition(g);
        if (g->has_op) upload_operator(g);
        return 0;
    }
    restrict_mesh_tables(g->mesh_full, ncells_prefix, nnodes_prefix, g->mesh);
    g->shrunk = true;
    upload_mesh(g);
    if (g->has_op) upload_operator(g);
    HMG_END
}

// The constrained set: the closure of the faces the caller names instead of the faces that belong to one cell.  No kernel knows
// that a constrained face lies on the outside -- the constraint is the per-cell entity bitmask every apply family fuses into its
// epilogue --, so the call forms the masks on the host and writes them into the device buffer the kernels already read (MeshDev
// travels by value: the pointer stays).  Towards everything cached it is a new operator: a pending r-update is formed first
// (with the masks it was recorded under), hmg_fcg objects need a new start, the Jacobi smoother's diagonal and the level-1
// system are formed again; the class-weight cache does not depend on the masks and is kept.
int hmg_grid_set_dirichlet_faces(hmg_grid *g, int64_t nfaces, const int64_t *faces)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(!g->part, "hmg_grid_set_dirichlet_faces: a partitioned grid keeps the default set (the faces that belong to one cell of the "
                   "whole mesh)");
    need(!g->shrunk, "hmg_grid_set_dirichlet_faces: the grid has been shrunk; a shrunk grid keeps the default set of its prefix");
    need(nfaces >= -1, "hmg_grid_set_dirichlet_faces: nfaces must be -1 (the default set), 0 (no constraint) or the number of faces");
    need(nfaces <= 0 || faces != nullptr, "hmg_grid_set_dirichlet_faces: null face list");
    MeshTables &M = g->mesh_full;
    // (everything is checked before anything changes)
    const std::vector<int32_t> dflt = boundary_faces(M);
    std::vector<int32_t> set = nfaces < 0 ? dflt : normalize_dirichlet_faces(M, nfaces, faces);
    if (g->ctx) {
        HIPCHK(hipSetDevice(g->ctx->device));
        materialize_r(g);
    }
    set_dirichlet_closure(M, set);
    g->dir_custom = set != dflt;                 // (the default set named face by face is the default set)
    if (g->dir_custom)
        g->dir_faces.swap(set);
    else
        g->dir_faces.clear();
    std::vector<uint16_t> dm = M.dmask;          // (padded as build_mesh_kernel_tables pads it)
    if (dm.size() & 1) dm.push_back((uint16_t)0);
    if (g->ctx) {
        need(g->d_dmask.p != nullptr && g->d_dmask.n == dm.size(), "hmg_grid_set_dirichlet_faces: the grid has no mask buffer of this size");
        HIPCHK(hipMemcpyAsync(g->d_dmask.p, dm.data(), dm.size() * sizeof(uint16_t), hipMemcpyHostToDevice, g->ctx->stream));
        HIPCHK(hipStreamSynchronize(g->ctx->stream));
    } else {
        DryUploads dry_scope(true, &g->upload_hash);
        DryUploads::note(dm.data(), dm.size() * sizeof(uint16_t));
    }
    g->op_epoch += 1;
    g->dinv_ready = false;
    g->coarse_ready = false;
    HMG_END
}

// The level-1 matrix with the constants in its kernel is solved on their complement (coarse_pcg_on_range) instead of being refused.
// Towards what is cached the flag is part of the operator, as the constrained set is.
int hmg_grid_set_mean_free(hmg_grid *g, int on)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(on == 0 || on == 1, "hmg_grid_set_mean_free: on must be 0 or 1");
    if (g->ctx) {
        HIPCHK(hipSetDevice(g->ctx->device));
        materialize_r(g);                        // (settles pending x-updates first)
    }
    g->mean_free = on != 0;
    g->op_epoch += 1;
    g->coarse_ready = false;
    HMG_END
}

int hmg_grid_mean_free(const hmg_grid *g) { return g ? (g->mean_free ? 1 : 0) : -1; }

int64_t hmg_grid_dirichlet_faces(const hmg_grid *g, int64_t *out, int64_t cap)
{
    if (!g) return -1;
    try {
        const std::vector<int32_t> dflt = g->dir_custom ? std::vector<int32_t>() : boundary_faces(g->part ? g->part->global : g->cur());
        const std::vector<int32_t> &set = g->dir_custom ? g->dir_faces : dflt;
        if (out)
            for (size_t q = 0; q < set.size() && (int64_t)q < cap; ++q) out[q] = (int64_t)set[q] + 1;
        return (int64_t)(set.size() / (size_t)g->dim);
    } catch (const std::exception &e) {
        last_error() = e.what();
        return -1;
    }
}

int64_t hmg_grid_ncells(const hmg_grid *g) { return g ? g->md.ncells : -1; }
int64_t hmg_grid_nnodes(const hmg_grid *g) { return g ? g->md.nnodes : -1; }
int hmg_grid_nlevels(const hmg_grid *g) { return g ? g->nlevels : -1; }
int64_t hmg_grid_nf(const hmg_grid *g, int level)
{
    return (g && level >= 1 && level <= g->nlevels) ? g->lt[level - 1].nf : -1;
}
int64_t hmg_grid_ld(const hmg_grid *g, int level)
{
    return (g && level >= 1 && level <= g->nlevels) ? g->lt[level - 1].ld : -1;
}

int hmg_grid_table_i32(const hmg_grid *g, int level, const char *which, int32_t *out, int64_t cap, int64_t *count)
{
    HMG_TRY
    need(g && which && count, "null argument");
    std::string w(which);
    std::vector<int32_t> tmp;
    const std::vector<int32_t> *src = nullptr;
    if (w == "dmask" || w == "dupmask") {
        const auto &m = w == "dmask" ? g->cur().dmask : g->cur().dupmask;
        tmp.assign(m.begin(), m.end());
        src = &tmp;
    } else if (w == "cell_class") {    // the cell's class in the class-weight cache; empty: this operator has no class table
        if (g->md.cell_class || !g->ctx) src = &g->cell_class;
        else src = &tmp;
    } else if (w == "upload_hash") {   // host-only grids: checksum of every table a device grid would have uploaded so far (two halves)
        tmp = {(int32_t)(uint32_t)(g->upload_hash & 0xffffffffu), (int32_t)(uint32_t)(g->upload_hash >> 32)};
        src = &tmp;
    } else if (w == "face_pairs") {
        src = &g->cur().face_pairs;
    } else if (w == "edge_ptr") {
        src = &g->cur().edge_ptr;
    } else if (w == "edge_ent") {
        src = &g->cur().edge_ent;
    } else if (w == "node_ptr") {
        src = &g->cur().node_ptr;
    } else if (w == "node_ent") {
        src = &g->cur().node_ent;
    } else if (w == "node_first") {
        src = &g->cur().node_first;
    } else if (w == "coarse_rowptr") {
        src = &g->cm.rowptr;
    } else if (w == "coarse_colidx") {
        src = &g->cm.colidx;
    } else if (w == "part_cells") {
        need(g->part != nullptr, "not a partitioned grid");
        src = &g->part->cells_g;
    } else if (w == "part_nodes") {
        need(g->part != nullptr, "not a partitioned grid");
        src = &g->part->nodes_g;
    } else if (w == "part_owned") {
        need(g->part != nullptr, "not a partitioned grid");
        src = &g->part->owned_node;
    } else if (w == "cut_counts") {
        need(g->part != nullptr, "not a partitioned grid");
        tmp = {(int32_t)g->part->nglobal[0], (int32_t)g->part->nglobal[1], (int32_t)g->part->nglobal[2],
               (int32_t)g->part->gid[0].size(), (int32_t)g->part->gid[1].size(), (int32_t)g->part->gid[2].size(),
               (int32_t)g->cur().ncut_face_pairs, (int32_t)g->cur().ncut_edge_groups, (int32_t)g->cur().ncut_node_groups,
               (int32_t)g->cur().cells_cut.size(), (int32_t)g->cur().cells_inner.size()};
        src = &tmp;
    } else if (w == "seg_ptr" || w == "seg_members" || w == "seg_counts") {
        need(g->part != nullptr, "not a partitioned grid");
        if (w == "seg_ptr") tmp.push_back(0);
        for (const auto &S : g->part->segs) {
            if (w == "seg_ptr")
                tmp.push_back(tmp.back() + (int32_t)S.members.size());
            else if (w == "seg_members")
                tmp.insert(tmp.end(), S.members.begin(), S.members.end());
            else
                for (int k = 0; k < 3; ++k) tmp.push_back((int32_t)S.count[k]);
        }
        src = &tmp;
    } else if (w == "cut_seg_faces" || w == "cut_seg_edges" || w == "cut_seg_nodes" || w == "cut_sidx_faces" ||
               w == "cut_sidx_edges" || w == "cut_sidx_nodes") {
        need(g->part != nullptr, "not a partitioned grid");
        const int k = w.find("faces") != std::string::npos ? 0 : w.find("edges") != std::string::npos ? 1 : 2;
        if (w.find("sidx") != std::string::npos)
            tmp.assign(g->part->seg_idx[k].begin(), g->part->seg_idx[k].end());
        else
            tmp = g->part->seg_of[k];
        src = &tmp;
    } else if (w == "cut_gid_faces" || w == "cut_gid_edges" || w == "cut_gid_nodes" || w == "cut_ent_faces" ||
               w == "cut_ent_edges" || w == "cut_ent_nodes") {
        need(g->part != nullptr, "not a partitioned grid");
        const int k = w.find("faces") != std::string::npos ? 0 : w.find("edges") != std::string::npos ? 1 : 2;
        if (w.find("gid") != std::string::npos)
            tmp.assign(g->part->gid[k].begin(), g->part->gid[k].end());
        else
            tmp = g->part->cell_lid[k];
        src = &tmp;
    } else if (w == "mult") {
        tmp.assign(g->cur().mult.begin(), g->cur().mult.end());
        src = &tmp;
    } else if (w == "interior_nodes") {
        const MeshTables &M = g->cur();
        for (int64_t i = 0; i < M.nnodes; ++i)
            if (!M.node_on_boundary[i] && M.node_first[i] >= 0) tmp.push_back((int32_t)i);
        src = &tmp;
    } else {
        need(level >= 1 && level <= g->nlevels, "level out of range");
        const LevelTables &T = g->lt[level - 1];
        if (w == "hier2slot")
            src = &T.hier2slot;
        else if (w == "slot_ijk")
            src = &T.slot_ijk;
        else if (w == "ref_cells")
            src = &T.ref_cells;
        else if (w == "elem_mask") {   // per slot: which Kuhn simplices with their lowest vertex there are fine elements (hmg_extrema.cpp)
            const auto &mk = g->fields.elem.at(level - 1).mask;
            tmp.assign(mk.begin(), mk.end());
            src = &tmp;
        } else if (w == "elem_dirs")   // ... and their lattice basis in slot_ijk coordinates, dim x dim
            src = &g->fields.elem.at(level - 1).dirs;
        else if (w == "par_a")
            src = &T.par_a;
        else if (w == "par_b")
            src = &T.par_b;
        else if (w == "rptr")
            src = &T.rptr;
        else if (w == "ridx")
            src = &T.ridx;
        else if (w == "slot_cls") {
            tmp.assign(T.slot_cls.begin(), T.slot_cls.end());
            src = &tmp;
        } else if (w == "layout") {
            tmp = {T.nf, T.ld, T.ncorner, T.nedge, T.nface, T.nei, T.nfi, T.nint, T.off_edge, T.off_face, T.off_int,
                   T.ncls, T.ndir, T.nterm, T.lds_g0, T.lds_g1, T.m};
            src = &tmp;
        } else
            throw std::runtime_error("unknown i32 table: " + w);
    }
    *count = (int64_t)src->size();
    if (out) {
        need(cap >= *count, "output buffer too small");
        std::copy(src->begin(), src->end(), out);
    }
    HMG_END
}

int hmg_grid_table_f64(const hmg_grid *g, int level, const char *which, double *out, int64_t cap, int64_t *count)
{
    HMG_TRY
    need(g && which && count, "null argument");
    std::string w(which);
    const std::vector<double> *src = nullptr;
    if (w == "coef")
        src = &g->coef;
    else if (w == "ctab") {
        need(level >= 1 && level <= g->nlevels, "level out of range");
        src = &g->lt[level - 1].ctab;
    } else if (w == "coarse_val")
        src = &g->cm.val;
    else if (w == "load") {
        need(level >= 1 && level <= g->nlevels, "level out of range");
        src = &g->lt[level - 1].load;
    }
#ifdef HMG_PHASE_TIMING
    else if (w == "phase_stamps") {
        need(g->ctx != nullptr, "no device");
        *count = (int64_t)g->d_blockpart.n;
        if (out) {
            need(cap >= *count, "output buffer too small");
            HIPCHK(hipStreamSynchronize(g->ctx->stream));
            HIPCHK(hipMemcpy(out, g->d_blockpart.p, sizeof(double) * g->d_blockpart.n, hipMemcpyDeviceToHost));
        }
        return 0;
    }
#endif
    else
        throw std::runtime_error("unknown f64 table: " + w);
    *count = (int64_t)src->size();
    if (out) {
        need(cap >= *count, "output buffer too small");
        std::copy(src->begin(), src->end(), out);
    }
    HMG_END
}

int hmg_grid_set_cut(hmg_grid *g, int64_t ngf, int64_t nge, int64_t ngn, int64_t nlf, const int64_t *face_gid,
                     const int32_t *face_cell_lid, int64_t nle, const int64_t *edge_gid, const int32_t *edge_cell_lid,
                     int64_t nln, const int64_t *node_gid, const int32_t *node_cell_lid)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    if (g->ctx) materialize_r(g);                // (a pending r-update was recorded for a grid without sums over ranks)
    // (a host-made cut list knows global ids only: all-reduce over the global cut buffer)
    g->sharers = false;
    set_cut_kind(g, 0, ngf, nlf, face_gid, face_cell_lid, nullptr, nullptr);
    set_cut_kind(g, 1, nge, nle, edge_gid, edge_cell_lid, nullptr, nullptr);
    set_cut_kind(g, 2, ngn, nln, node_gid, node_cell_lid, nullptr, nullptr);
    HMG_END
}

}  // extern "C"
