// Multi-GPU: the cut exchange of a partitioned grid (buffer layouts, pack, sum over the ranks), the in-library RCCL
// communicator and the built-in exchange callbacks; with the entry points that front them (hmg_comm_*, hmg_grid_set_exchange*,
// hmg_grid_set_overlap, hmg_grid_use_comm, hmg_grid_cut_*, hmg_grid_exchange_messages).
#include "../../include/hmg.h"
#include "hmg_objects.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace hmg {
namespace {

// Buffer layout of one level (see CutLevel), built at the first exchange on that level and after every re-partition.
CutLevel &cut_level(hmg_grid *g, const LevelDev &lv)
{
    if (g->cutlv.size() != (size_t)g->nlevels) {
        g->cutlv.clear();
        for (int l = 0; l < g->nlevels; ++l) g->cutlv.emplace_back(new CutLevel);
    }
    CutLevel &C = *g->cutlv[lv.level - 1];
    if (C.ready) return C;
    const int64_t per[3] = {lv.nfi, lv.nei, 1};
    DryUploads dry_scope(!g->ctx, &g->upload_hash);
    hipStream_t st = g->ctx ? g->ctx->stream : nullptr;
    std::vector<int64_t> pos;
    if (!g->sharers) {
        need(!g->part || g->part->global_ids,
             "this partition was analysed on the rank's halo only: its cut ids mean nothing to other ranks -- exchange among "
             "the sharers (hmg_grid_use_comm / hmg_grid_set_exchange_p2p) or create the grid with HMG_PARTITION_ANALYSIS=global");
        int64_t off = 0;
        for (int k = 0; k < 3; ++k) {
            pos.resize(g->cut[k].gid.size());
            for (size_t e = 0; e < pos.size(); ++e) pos[e] = off + g->cut[k].gid[e] * per[k];
            C.pos[k].upload(pos, st);
            off += g->cut[k].nglobal * per[k];
        }
        C.ndoubles = off;
    } else {
        need(g->part != nullptr, "the sharers-only exchange needs the library's own partition analysis");
        const Partition &P = *g->part;
        const size_t nseg = P.segs.size();
        std::vector<int64_t> soff(nseg + 1, 0);
        for (size_t q = 0; q < nseg; ++q)
            soff[q + 1] = soff[q] + P.segs[q].count[0] * per[0] + P.segs[q].count[1] * per[1] + P.segs[q].count[2] * per[2];
        for (int k = 0; k < 3; ++k) {
            pos.resize(g->cut[k].seg.size());
            for (size_t e = 0; e < pos.size(); ++e) {
                const Partition::Segment &S = P.segs[(size_t)g->cut[k].seg[e]];
                const int64_t kbase = k == 0 ? 0 : k == 1 ? S.count[0] * per[0] : S.count[0] * per[0] + S.count[1] * per[1];
                pos[e] = soff[(size_t)g->cut[k].seg[e]] + kbase + g->cut[k].sidx[e] * per[k];
            }
            C.pos[k].upload(pos, st);
        }
        C.ndoubles = soff[nseg];
        // messages (one per segment and peer) and the summation plan: every member adds the members' partial segments in
        // ascending rank order, its own from the buffer, the others' from the staging area -- the same bits on every member
        C.ops.clear();
        std::vector<int64_t> plan{(int64_t)nseg}, mtab;
        plan.resize(1 + 4 * nseg);
        int64_t stage = 0;
        for (size_t q = 0; q < nseg; ++q) {
            const Partition::Segment &S = P.segs[q];
            const int64_t size = soff[q + 1] - soff[q];
            plan[1 + 4 * q] = soff[q];
            plan[2 + 4 * q] = size;
            plan[3 + 4 * q] = (int64_t)S.members.size();
            plan[4 + 4 * q] = (int64_t)mtab.size();
            for (int32_t m : S.members) {
                if (m == P.rank) {
                    mtab.push_back(-1);
                    continue;
                }
                mtab.push_back(stage);
                if (size > 0) {
                    C.ops.push_back(m);
                    C.ops.push_back(soff[q]);
                    C.ops.push_back(size);
                    C.ops.push_back(stage);
                }
                stage += size;
            }
        }
        C.nstage = stage;
        for (size_t q = 0; q < nseg; ++q) plan[4 + 4 * q] += (int64_t)(1 + 4 * nseg);    // absolute offsets of the member tables
        plan.insert(plan.end(), mtab.begin(), mtab.end());
        C.plan.upload(plan, st);
    }
    C.ready = true;
    return C;
}

int64_t cut_doubles(hmg_grid *g, const LevelDev &lv) { return cut_level(g, lv).ndoubles; }

}  // namespace

// unpack = 0: buffer <- first local copy of every cut entity;  unpack = 1: every local copy <- buffer
void cut_pack(hmg_grid *g, const LevelDev &lv, double *x, int unpack)
{
    const Launch &L = g->ctx->L;
    CutLevel &C = cut_level(g, lv);
    CutPackArgs a{};
    for (int k = 0; k < 3; ++k) {
        a.n[k] = g->cut[k].nentries;
        a.pos[k] = C.pos[k].p;
        a.cell_lid[k] = g->cut[k].cell_lid.p;
        a.first[k] = g->cut[k].first.p;
    }
    launch_cut_pack(L, lv, a, g->ex_buf, x, unpack);
}

// The sum over ranks of the packed buffer, started (begin) and joined (finish) -- or both at once on the context's stream.
// Global layout: one in-place all-reduce (positions no local copy writes must be zero: filled first).  Segment layout:
// the partial segments travel to the other members, then every member adds them up in rank order.
void exchange_prepare(hmg_grid *g, const LevelDev &lv)
{
    CutLevel &C = cut_level(g, lv);
    need(C.ndoubles <= g->ex_cap, "exchange buffer too small for this level");
    if (g->sharers)
        need(C.nstage <= g->stage_cap, "staging buffer too small for this level");
    else
        launch_fill(g->ctx->L, g->ex_buf, C.ndoubles, 0.0);
}

void exchange_run(hmg_grid *g, const LevelDev &lv, bool async)
{
    CutLevel &C = cut_level(g, lv);
    int rc;
    if (g->sharers) {
        hmg_p2p_fn f = async ? g->p2p_begin : g->p2p;
        need(f != nullptr, "sharers-only exchange: no p2p transport set (hmg_grid_use_comm / hmg_grid_set_exchange_p2p)");
        rc = f(g->ex_user, g->ex_buf, g->stage, (int64_t)C.ops.size() / 4, C.ops.data());
    } else if (async)
        rc = g->ex_begin(g->ex_user, g->ex_buf, C.ndoubles);
    else if (g->exchange)
        rc = g->exchange(g->ex_user, g->ex_buf, C.ndoubles);
    else
        rc = g->ex_begin(g->ex_user, g->ex_buf, C.ndoubles) || g->ex_end(g->ex_user);
    if (rc != 0) throw std::runtime_error("exchange callback failed");
}

void exchange_finish(hmg_grid *g, const LevelDev &lv, bool async)
{
    if (async && g->ex_end(g->ex_user) != 0) throw std::runtime_error("exchange (end) callback failed");
    if (g->sharers) {
        CutLevel &C = cut_level(g, lv);
        launch_seg_sum(g->ctx->L, C.plan.p, C.ndoubles, g->ex_buf, g->stage);
    }
}

void exchange_cut(hmg_grid *g, const LevelDev &lv, double *x)
{
    if (cut_doubles(g, lv) == 0) return;
    exchange_prepare(g, lv);
    cut_pack(g, lv, x, 0);
    exchange_run(g, lv, false);
    exchange_finish(g, lv, false);
    cut_pack(g, lv, x, 1);
}

// ---- in-library communicator: RCCL, resolved at run time ------------------------------------------
// librccl is opened with dlopen when a communicator is first asked for (a host process that already holds a copy --
// torch bundles one -- shares it), so the library loads and runs single-GPU without RCCL present.
namespace {

struct RcclApi {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi &rccl()
{
    static RcclApi api;
    if (api.h) return api;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names)
        if ((api.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!api.h)
        for (const char *n : names)
            if ((api.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!api.h) throw std::runtime_error(std::string("RCCL not found (dlopen librccl.so.1): ") + dlerror());
    auto sym = [&](const char *n) {
        void *p = dlsym(api.h, n);
        if (!p) throw std::runtime_error(std::string("RCCL symbol missing: ") + n);
        return p;
    };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    return api;
}

void nccl_check(ncclResult_t r, const char *what)
{
    if (r != ncclSuccess) throw std::runtime_error(std::string("RCCL error in ") + what + ": " + rccl().GetErrorString(r));
}

// in-place sum over ranks of n doubles, enqueued on `s`
void comm_allreduce(hmg_ctx *c, double *buf, int64_t n, hipStream_t s)
{
    need(c->comm != nullptr, "this context's communicator has been destroyed (hmg_comm_destroy)");
    nccl_check(rccl().AllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, c->comm, s), "ncclAllReduce");
    c->comm_calls += 1;
    c->comm_doubles += n;
}

// The messages of one sharers-only exchange as ONE grouped RCCL call: per message a send of this rank's partial segment and
// a receive of the peer's into the staging area.  Two members of a segment list their common segments in the same order
// (Partition::segs), and RCCL matches the k-th send a -> b with the k-th receive of b from a.
void comm_p2p(hmg_ctx *c, double *buf, double *stage, int64_t nmsg, const int64_t *m, hipStream_t s)
{
    if (nmsg == 0) return;
    need(c->comm != nullptr, "this context's communicator has been destroyed (hmg_comm_destroy)");
    int64_t sent = 0;
    nccl_check(rccl().GroupStart(), "ncclGroupStart");
    for (int64_t i = 0; i < nmsg; ++i) {
        // (rehearsal of one rank's share of a larger partition: every peer is this rank itself -- a local copy stands in
        //  for the link)
        const int peer = c->comm_rehearsal ? c->comm_rank : (int)m[4 * i];
        const size_t n = (size_t)m[4 * i + 2];
        nccl_check(rccl().Send(buf + m[4 * i + 1], n, ncclDouble, peer, c->comm, s), "ncclSend");
        nccl_check(rccl().Recv(stage + m[4 * i + 3], n, ncclDouble, peer, c->comm, s), "ncclRecv");
        sent += (int64_t)n;
    }
    nccl_check(rccl().GroupEnd(), "ncclGroupEnd");
    c->comm_calls += 1;
    c->comm_doubles += sent;
}

// The built-in forms of the exchange callbacks (user = the grid): everything is enqueued on HIP streams, no host
// synchronisation and no foreign code between two kernels of a V-cycle.  A callback reports through its return value.
template <class F>
int guarded(F f)
{
    try {
        f();
    } catch (const std::exception &e) {
        last_error() = e.what();
        return 1;
    }
    return 0;
}

// the asynchronous forms: `issue` runs on the second stream behind the pack kernels, and ev_summed marks its end
template <class F>
int on_comm_stream(hmg_ctx *c, F issue)
{
    return guarded([&] {
        need(c->comm != nullptr, "this context's communicator has been destroyed (hmg_comm_destroy)");
        HIPCHK(hipEventRecord(c->ev_packed, c->stream));
        HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_packed, 0));
        issue();
        HIPCHK(hipEventRecord(c->ev_summed, c->comm_stream));
    });
}

int comm_p2p_sync(void *user, void *buf, void *stage, int64_t nmsg, const int64_t *msgs)
{
    hmg_ctx *c = ((hmg_grid *)user)->ctx;
    return guarded([&] { comm_p2p(c, (double *)buf, (double *)stage, nmsg, msgs, c->stream); });
}

int comm_p2p_begin(void *user, void *buf, void *stage, int64_t nmsg, const int64_t *msgs)
{
    hmg_ctx *c = ((hmg_grid *)user)->ctx;
    return on_comm_stream(c, [&] { comm_p2p(c, (double *)buf, (double *)stage, nmsg, msgs, c->comm_stream); });
}

int comm_exchange(void *user, void *buf, int64_t n)
{
    hmg_ctx *c = ((hmg_grid *)user)->ctx;
    return guarded([&] { comm_allreduce(c, (double *)buf, n, c->stream); });
}

int comm_exchange_begin(void *user, void *buf, int64_t n)
{
    hmg_ctx *c = ((hmg_grid *)user)->ctx;
    return on_comm_stream(c, [&] { comm_allreduce(c, (double *)buf, n, c->comm_stream); });
}

int comm_exchange_end(void *user)
{
    hmg_ctx *c = ((hmg_grid *)user)->ctx;
    return guarded([&] { HIPCHK(hipStreamWaitEvent(c->stream, c->ev_summed, 0)); });
}

}  // namespace

void comm_drop(hmg_ctx *c)
{
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
    if (c->ev_summed) (void)hipEventDestroy(c->ev_summed);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    c->comm = nullptr;
    c->comm_nranks = 1;
    c->comm_rank = 0;
    c->ev_packed = c->ev_summed = nullptr;
    c->comm_stream = nullptr;
}

}  // namespace hmg

extern "C" {

int hmg_grid_set_exchange(hmg_grid *g, hmg_exchange_fn exchange, hmg_exchange_fn scalar_sum_fn, void *user,
                          void *device_exchange_buf, int64_t exchange_buf_doubles)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    if (g->ctx) materialize_r(g);                // (a pending r-update was recorded for a grid without sums over ranks)
    g->exchange = exchange;
    g->scalar_sum = scalar_sum_fn;
    g->cut_agreed_ready = false;
    g->dinv_ready = false;                       // (the smoother's diagonal is summed through the exchange)
    g->ex_user = user;
    g->ex_buf = (double *)device_exchange_buf;
    g->ex_cap = exchange_buf_doubles;
    HMG_END
}

int hmg_grid_set_exchange_async(hmg_grid *g, hmg_exchange_fn begin, int (*end)(void *user))
{
    HMG_TRY
    need(g != nullptr, "null grid");
    if (g->ctx) materialize_r(g);                // (a pending r-update was recorded for a grid without sums over ranks)
    g->ex_begin = begin;
    g->ex_end = end;
    g->dinv_ready = false;
    HMG_END
}

int hmg_grid_set_overlap(hmg_grid *g, int enabled)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    g->overlap = enabled != 0;
    HMG_END
}

int hmg_comm_unique_id(void *out128)
{
    HMG_TRY
    need(out128 != nullptr, "null argument");
    ncclUniqueId id;
    nccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
    static_assert(sizeof(id) == HMG_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(out128, &id, sizeof(id));
    HMG_END
}

int hmg_comm_init(hmg_ctx *ctx, int nranks, int rank, const void *unique_id128)
{
    HMG_TRY
    need(ctx && unique_id128, "null argument");
    need(nranks >= 1 && rank >= 0 && rank < nranks, "rank out of range");
    need(ctx->comm == nullptr, "this context already has a communicator");
    HIPCHK(hipSetDevice(ctx->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id128, sizeof(id));
    nccl_check(rccl().CommInitRank(&ctx->comm, nranks, id, rank), "ncclCommInitRank");
    ctx->comm_nranks = nranks;
    ctx->comm_rank = rank;
    HIPCHK(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_packed, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_summed, hipEventDisableTiming));
    HMG_END
}

int hmg_comm_destroy(hmg_ctx *ctx)
{
    HMG_TRY
    need(ctx != nullptr, "null ctx");
    if (ctx->comm) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->comm_stream));
        nccl_check(rccl().CommDestroy(ctx->comm), "ncclCommDestroy");
        ctx->comm = nullptr;
        // the second stream and its events go with the communicator (a later hmg_comm_init makes new ones); grids that
        // still point at the built-in exchange callbacks fail cleanly in comm_allreduce / comm_p2p from now on
        comm_drop(ctx);
    }
    HMG_END
}

int hmg_comm_stats(hmg_ctx *ctx, int64_t *calls, int64_t *doubles)
{
    HMG_TRY
    need(ctx && calls && doubles, "null argument");
    *calls = ctx->comm_calls;
    *doubles = ctx->comm_doubles;
    HMG_END
}

int hmg_comm_sum_host(hmg_ctx *ctx, double *vals, int count)
{
    HMG_TRY
    need(ctx && vals, "null argument");
    need(ctx->comm != nullptr, "hmg_comm_init must be called first");
    need(count >= 1 && count <= S_COUNT - S_HOST, "count must be 1..4");
    double *d = ctx->L.scal + S_HOST;     // (the last slots of the scalar bank are not used by the kernels)
    HIPCHK(hipMemcpyAsync(d, vals, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    comm_allreduce(ctx, d, count, ctx->stream);
    HIPCHK(hipMemcpyAsync(vals, d, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HMG_END
}

int64_t hmg_grid_cut_buffer_doubles(const hmg_grid *cg, int level)
{
    hmg_grid *g = const_cast<hmg_grid *>(cg);
    if (!g || level < 0 || level > g->nlevels) return -1;
    try {
        if (level == 0) {   // required capacity: max over levels and the coarse gather
            int64_t n = g->part ? g->part->global.nnodes : 0;
            for (int l = 0; l < g->nlevels; ++l) n = std::max(n, cut_doubles(g, g->ld[l]));
            return n;
        }
        return cut_doubles(g, g->ld[level - 1]);
    } catch (const std::exception &e) {
        last_error() = e.what();
        return -1;
    }
}

int64_t hmg_grid_cut_stage_doubles(const hmg_grid *cg)
{
    hmg_grid *g = const_cast<hmg_grid *>(cg);
    if (!g) return -1;
    try {
        int64_t n = 0;
        for (int l = 0; l < g->nlevels; ++l) n = std::max(n, cut_level(g, g->ld[l]).nstage);
        return n;
    } catch (const std::exception &e) {
        last_error() = e.what();
        return -1;
    }
}

int hmg_grid_use_comm(hmg_grid *g)
{
    HMG_TRY
    need(g && g->ctx, "null grid or host-only grid");
    need(g->ctx->comm != nullptr, "hmg_comm_init must be called on the grid's context first");
    need(g->part != nullptr, "not a partitioned grid (hmg_grid_create_partition)");
    need(g->ctx->comm_rehearsal || (g->part->nranks == g->ctx->comm_nranks && g->part->rank == g->ctx->comm_rank),
         "the grid's partition and the context's communicator disagree on rank / size");
    // exchange among the sharers of each cut entity (grouped ncclSend / ncclRecv) unless HMG_EXCHANGE=allreduce asks for
    // round 2's single all-reduce over the global cut buffer
    const char *mode = std::getenv("HMG_EXCHANGE");
    g->sharers = !(mode && std::string(mode) == "allreduce");
    g->cutlv.clear();
    const int64_t cap = std::max<int64_t>(hmg_grid_cut_buffer_doubles(g, 0), 1);
    g->own_exbuf.alloc((size_t)cap);
    g->ex_buf = g->own_exbuf.p;
    g->ex_cap = cap;
    const int64_t scap = std::max<int64_t>(hmg_grid_cut_stage_doubles(g), 1);
    g->own_stage.alloc((size_t)scap);
    g->stage = g->own_stage.p;
    g->stage_cap = scap;
    g->ex_user = g;
    g->exchange = comm_exchange;             // (the level-1 gather stays an all-reduce of the global nodal vector)
    g->scalar_sum = comm_exchange;           // (the same in-place sum, on the scalar bank)
    g->cut_agreed_ready = false;
    g->dinv_ready = false;
    g->ex_begin = comm_exchange_begin;
    g->ex_end = comm_exchange_end;
    g->p2p = comm_p2p_sync;
    g->p2p_begin = comm_p2p_begin;
    HMG_END
}

int hmg_grid_set_exchange_p2p(hmg_grid *g, int enabled, hmg_p2p_fn p2p, hmg_p2p_fn p2p_begin, void *device_stage_buf,
                              int64_t stage_buf_doubles)
{
    HMG_TRY
    need(g != nullptr, "null grid");
    need(!enabled || g->part != nullptr, "the sharers-only exchange needs a grid made by hmg_grid_create_partition");
    g->sharers = enabled != 0;
    g->cutlv.clear();
    g->dinv_ready = false;
    g->p2p = p2p;
    g->p2p_begin = p2p_begin;
    g->stage = (double *)device_stage_buf;
    g->stage_cap = stage_buf_doubles;
    HMG_END
}

int hmg_grid_exchange_messages(const hmg_grid *cg, int level, int64_t *out, int64_t cap, int64_t *count)
{
    HMG_TRY
    hmg_grid *g = const_cast<hmg_grid *>(cg);
    need(g && count, "null argument");
    need(level >= 1 && level <= g->nlevels, "level out of range");
    const CutLevel &C = cut_level(g, g->ld[level - 1]);
    *count = (int64_t)C.ops.size();
    if (out) {
        need(cap >= *count, "output buffer too small");
        std::copy(C.ops.begin(), C.ops.end(), out);
    }
    HMG_END
}

}  // extern "C"
