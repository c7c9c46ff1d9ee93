"""
A record / replay transport for partitioned grids: an N-rank cut exchange run rank by rank in ONE process (test code only).

The library talks to its transport through callbacks (include/hmg.h: hmg_grid_set_exchange, hmg_grid_set_exchange_async,
hmg_grid_set_exchange_p2p, hmg_ctx_set_scalar_bank; dist.Exchange with backend "torch" is the model), and every rank issues its
callbacks in the same order: the j-th collective of rank a is the j-th of every rank.  So `run_world` runs PASSES.  In a pass every
rank in turn gets a fresh grid and runs the same body.  Collective j is REPLAYED -- answered with what the other ranks sent -- once
the records of all ranks for it exist from an earlier pass; the first collective without records is RECORDED (this rank's outgoing
data is kept) and, like every later one of that pass, answered with zeros.  Collectives 1 .. j-1 were answered exactly, so what a
rank sends in collective j is exact in the pass that records it: a body with K collectives is complete after K + 1 passes, and the
results of that last pass are those of a real N-rank run with this module's transport:

  p2p / p2p_begin   messages {peer, offset, count, staging offset}: the k-th message from a to b is answered with the data of the
                    k-th message from b to a (the rule of include/hmg.h), written to stage[staging offset .. + count); the staging
                    buffer is NaN everywhere else, before every callback;
  exchange / begin  (all-reduce layout) and scalar_sum: the sum of all ranks' buffers, added in ASCENDING RANK ORDER in float64 on
                    the host -- the definition of this transport's all-reduce;
  end               nothing: the data has landed when `begin` returns.

Fresh grids per pass are needed because the library caches what it learns from a collective (the agreed cut size of
agree_on_cut, csrc/hmg_smooth.cpp): a grid that was fed zeros once has cached a wrong size.  Every rank-run has its own scalar bank.
No torch.distributed, no process group.
"""
import ctypes

import numpy as np
import torch

from homogenization_jl_amd import _lib as L

COLLECTIVES = ("exchange", "begin", "p2p", "p2p_begin", "scalar_sum")
STAGE_PAD = 8            # NaN doubles behind the staging capacity the library is told: a read past the end shows up as well


class Replay:
    """What the passes of one run_world share: the exact records of the collectives replayed so far."""

    def __init__(self, world):
        self.world = world
        self.records = []        # records[j][rank]: dict(kind, count, data | buf, msgs)
        self.pending = {}        # rank -> this pass's record of collective len(records)


class Transport:
    """The callbacks of one rank-run.  sharers: the segment layout (hmg_grid_set_exchange_p2p(g, 1, ...)) or the all-reduce over the
    global cut buffer.  fault(rank, msgs, deliveries) -> deliveries: a deliberately wrong delivery (the harness' self-check);
    deliveries = [[staging offset, data], ...] in message order."""

    def __init__(self, replay, ctx, grid, sharers=True, fault=None):
        self.replay, self.ctx, self.grid, self.rank, self.fault = replay, ctx, grid, grid.rank, fault
        self.sharers = sharers
        self.kinds = []          # every callback of this run, `end` included
        self.ncoll = 0           # collectives so far
        self.complete = True     # every collective was replayed
        self.error = None        # the first exception inside a callback (none crosses the C boundary)
        self.delivered = None    # staging words the last p2p callback delivered
        self.sent = []           # (collective index, kind) -> what this run sent, for the checks
        lib = L.load()
        dev = torch.device("cuda", ctx.device)
        if sharers:              # (the segment layout decides the buffer sizes: switch it on before asking for them)
            L.check(lib.hmg_grid_set_exchange_p2p(grid.h, 1, L.P2P_FN(0), L.P2P_FN(0), None, 0))
        else:
            L.check(lib.hmg_grid_set_exchange_p2p(grid.h, 0, L.P2P_FN(0), L.P2P_FN(0), None, 0))
        n = max(grid.exchange_doubles(), 1)
        self.buf = torch.zeros(n, dtype=torch.float64, device=dev)
        self.scal = torch.zeros(16, dtype=torch.float64, device=dev)
        L.check(lib.hmg_ctx_set_scalar_bank(ctx.h, ctypes.c_void_p(self.scal.data_ptr())))
        sh = ctx.stream_handle()
        self._stream = torch.cuda.ExternalStream(sh, device=dev) if sh else torch.cuda.default_stream(dev)
        self._cb = (L.EXCHANGE_FN(self._guard(self._exchange)), L.EXCHANGE_FN(self._guard(self._scalar)),
                    L.EXCHANGE_FN(self._guard(self._begin)), L.EXCHANGE_END_FN(self._guard(self._end)),
                    L.P2P_FN(self._guard(self._p2p)), L.P2P_FN(self._guard(self._p2p_begin)))
        self._held = [self.buf, self.scal, self._cb]
        L.check(lib.hmg_grid_set_exchange(grid.h, self._cb[0], self._cb[1], None, ctypes.c_void_p(self.buf.data_ptr()), n))
        L.check(lib.hmg_grid_set_exchange_async(grid.h, self._cb[2], self._cb[3]))
        self.stage = None
        if sharers:
            self.nstage = max(int(lib.hmg_grid_cut_stage_doubles(grid.h)), 1)
            self.stage = torch.full((self.nstage + STAGE_PAD,), float("nan"), dtype=torch.float64, device=dev)
            self._held.append(self.stage)
            L.check(lib.hmg_grid_set_exchange_p2p(grid.h, 1, self._cb[4], self._cb[5], ctypes.c_void_p(self.stage.data_ptr()),
                                                  self.nstage))
        ctx._keepalive += self._held                              # the library points into them as long as the grid lives

    def release(self):
        """After the grid is gone and the context has its own scalar bank back: nothing points into this run's memory."""
        for obj in self._held:
            self.ctx._keepalive[:] = [o for o in self.ctx._keepalive if o is not obj]
        self._held = []

    def set_overlap(self, enabled):
        L.check(L.load().hmg_grid_set_overlap(self.grid.h, 1 if enabled else 0))

    def stage_readback(self):
        """(staging buffer as it is now, which of its words the last p2p callback delivered)"""
        if self.stage is None:
            return None, None
        with torch.cuda.stream(self._stream):
            host = self.stage.cpu().numpy().copy()
        mask = self.delivered if self.delivered is not None else np.zeros(host.size, dtype=bool)
        return host, mask

    # -- the callbacks ----------------------------------------------------------------------------------------------------
    def _guard(self, fn):
        def wrapped(*args):
            try:
                fn(*args)
                return 0
            except BaseException as e:          # never let an exception cross the C boundary
                if self.error is None:
                    self.error = e
                return 1
        return wrapped

    def _collective(self, kind, record):
        """The records of all ranks for this collective (replay), or None after keeping `record` (this pass records or is past the
        first collective it could not replay)."""
        R = self.replay
        j = self.ncoll
        self.ncoll += 1
        self.kinds.append(kind)
        record["kind"] = kind
        self.sent.append(record)
        if j < len(R.records):
            recs = R.records[j]
            mine = recs[self.rank]
            assert mine["kind"] == kind, f"rank {self.rank}, collective {j}: {kind} now, {mine['kind']} when it was recorded"
            for key in ("data", "buf"):          # the same run sends the same bits again: what the peers were given is what it sent
                if key in record:
                    np.testing.assert_array_equal(record[key], mine[key], err_msg=f"rank {self.rank}, collective {j}: not reproducible")
            return recs
        self.complete = False
        if j == len(R.records):
            R.pending[self.rank] = record
        return None

    def _sum(self, kind, tensor, ptr, count):
        off = (ptr - tensor.data_ptr()) // 8
        assert 0 <= off and off + count <= tensor.numel(), (kind, off, count)
        with torch.cuda.stream(self._stream):          # behind the pack kernels, before the unpack kernels
            view = tensor[off:off + count]
            recs = self._collective(kind, {"count": int(count), "data": view.cpu().numpy().copy()})
            if recs is None:
                view.zero_()
                return
            total = None
            for r in range(self.replay.world):                           # ascending rank order, float64, on the host
                assert recs[r]["kind"] == kind and recs[r]["count"] == count, (kind, count, r, recs[r]["kind"], recs[r]["count"])
                total = recs[r]["data"].copy() if total is None else total + recs[r]["data"]
            view.copy_(torch.from_numpy(total))

    def _exchange(self, user, ptr, count):
        self._sum("exchange", self.buf, ptr, count)

    def _begin(self, user, ptr, count):
        self._sum("begin", self.buf, ptr, count)

    def _scalar(self, user, ptr, count):
        self._sum("scalar_sum", self.scal, ptr, count)

    def _end(self, user):
        self.kinds.append("end")

    def _p2p(self, user, ptr, sptr, nmsgs, msgs):
        self._messages("p2p", ptr, sptr, nmsgs, msgs)

    def _p2p_begin(self, user, ptr, sptr, nmsgs, msgs):
        self._messages("p2p_begin", ptr, sptr, nmsgs, msgs)

    def _messages(self, kind, ptr, sptr, nmsgs, msgs):
        m = np.ctypeslib.as_array(msgs, shape=(int(nmsgs) * 4,)).reshape(-1, 4).copy() if nmsgs else np.zeros((0, 4), np.int64)
        assert ptr == self.buf.data_ptr() and (not nmsgs or sptr == self.stage.data_ptr())
        with torch.cuda.stream(self._stream):
            full = self.buf.cpu().numpy().copy()
            for peer, off, cnt, soff in m:
                assert 0 <= peer < self.replay.world and peer != self.rank
                assert 0 <= off and off + cnt <= full.size and 0 <= soff and soff + cnt <= self.nstage, (peer, off, cnt, soff)
            recs = self._collective(kind, {"msgs": m, "buf": full})
            deliveries = []
            if recs is None:
                deliveries = [[int(soff), np.zeros(int(cnt))] for peer, off, cnt, soff in m]
            else:
                nth = {}
                for peer, off, cnt, soff in m:
                    pm = recs[peer]["msgs"]
                    back = pm[pm[:, 0] == self.rank]                     # the peer's messages to this rank, in its order
                    assert recs[peer]["kind"] == kind
                    assert len(back) == int((m[:, 0] == peer).sum()), f"ranks {self.rank} and {peer} list {int((m[:, 0] == peer).sum())} and {len(back)} messages"
                    k = nth.get(int(peer), 0)
                    nth[int(peer)] = k + 1
                    assert back[k, 2] == cnt, f"message {k} between ranks {self.rank} and {peer}: {cnt} and {back[k, 2]} doubles"
                    deliveries.append([int(soff), recs[peer]["buf"][back[k, 1]:back[k, 1] + cnt].copy()])
                for peer in range(self.replay.world):                    # nobody sends to a rank that does not expect it
                    pm = recs[peer]["msgs"]
                    assert peer == self.rank or int((pm[:, 0] == self.rank).sum()) == nth.get(peer, 0)
                if self.fault is not None:
                    deliveries = self.fault(self.rank, m, deliveries)
            host = np.full(self.nstage + STAGE_PAD, np.nan)             # poison: a read outside what was delivered shows up
            mask = np.zeros(host.size, dtype=bool)
            for soff, data in deliveries:
                assert 0 <= soff and soff + data.size <= host.size
                host[soff:soff + data.size] = data
                mask[soff:soff + data.size] = True
            self.delivered = mask
            self.stage.copy_(torch.from_numpy(host))


class World:
    """What run_world returns.  results[rank] / first[rank]: what the body returned in the last (complete) pass and in the first
    one, in which every collective was answered with zeros (None where the body failed on them); kinds[rank]: the callbacks of
    the last pass in order; records[j][rank]: what rank sent in collective j; stages[rank] = (staging buffer after the run,
    delivered words)."""


def run_world(ctx, world, make_rank, body, sharers=True, fault=None, max_passes=40):
    """make_rank(rank) -> a fresh dist.PartitionedGrid on ctx; body(rank, grid, transport) -> anything."""
    lib = L.load()
    R = Replay(world)
    out = World()
    out.first = None
    try:
        for npass in range(1, max_passes + 1):
            R.pending = {}
            results, kinds, stages, complete = [], [], [], True
            for rank in range(world):
                grid = make_rank(rank)
                assert grid.rank == rank and grid.nranks == world
                t = Transport(R, ctx, grid, sharers=sharers, fault=fault)
                try:
                    res = body(rank, grid, t)
                except L.HmgError:
                    if t.error is not None:
                        raise t.error
                    if t.complete:
                        raise
                    res = None                  # (a run that was fed zeros may stumble over them: the next pass knows more)
                if t.error is not None:
                    raise t.error
                ctx.sync()
                results.append(res)
                kinds.append(t.kinds)
                stages.append(t.stage_readback())
                complete = complete and t.complete
                L.check(lib.hmg_ctx_set_scalar_bank(ctx.h, None))
                grid.close()
                t.release()
            if out.first is None:
                out.first = results
            if complete:
                assert not R.pending
                for rank in range(1, world):    # the library's promise; a deadlock on real hardware is what breaks otherwise
                    assert kinds[rank] == kinds[0], f"ranks 0 and {rank} issued different callbacks: {kinds[0]} / {kinds[rank]}"
                out.results, out.kinds, out.stages, out.records, out.passes = results, kinds, stages, R.records, npass
                assert npass == len([k for k in kinds[0] if k in COLLECTIVES]) + 1
                return out
            j = len(R.records)
            assert sorted(R.pending) == list(range(world)), f"collective {j} was issued by ranks {sorted(R.pending)} only"
            rec = [R.pending[r] for r in range(world)]
            assert len({r["kind"] for r in rec}) == 1, f"collective {j}: " + ", ".join(r["kind"] for r in rec)
            R.records.append(rec)
        raise AssertionError(f"more than {max_passes} passes")
    finally:
        L.check(lib.hmg_ctx_set_scalar_bank(ctx.h, None))


# ---- the buffer layout of the segment form, from the library's tables (as tests/test_dist_gloo.py builds it) -----------------
def entity_layout(g, level):
    lay = g.table_i32("layout", level)
    return {"nfi": int(lay[6]), "nei": int(lay[5]), "off_edge": int(lay[8]), "off_face": int(lay[9]),
            "s2h": np.argsort(g.table_i32("hier2slot", level))}


def cut_layout(g, level):
    """Where every local copy of a cut DOF lies -- (rows, cols) in the level vector, dst in the exchange buffer of the segment form
    -- and the segments: members (ascending ranks), offset and size in this rank's buffer."""
    e = entity_layout(g, level)
    per = {"faces": e["nfi"], "edges": e["nei"], "nodes": 1}
    offs = {"faces": e["off_face"], "edges": e["off_edge"], "nodes": 0}
    sptr, smem = g.table_i32("seg_ptr"), g.table_i32("seg_members")
    scnt = g.table_i32("seg_counts").reshape(-1, 3).astype(np.int64)
    nseg = scnt.shape[0]
    size = scnt @ np.array([e["nfi"], e["nei"], 1], dtype=np.int64)
    soff = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    kbase = {"faces": np.zeros(nseg, np.int64), "edges": scnt[:, 0] * e["nfi"], "nodes": scnt[:, 0] * e["nfi"] + scnt[:, 1] * e["nei"]}
    rows, cols, dst, gids = [], [], [], []
    for code, kind in enumerate(("faces", "edges", "nodes")):
        sg = g.table_i32("cut_seg_" + kind).astype(np.int64)
        sx = g.table_i32("cut_sidx_" + kind).astype(np.int64)
        ce = g.table_i32("cut_ent_" + kind).astype(np.int64)
        gid = g.table_i32("cut_gid_" + kind).astype(np.int64)
        if per[kind] == 0 or sg.size == 0:
            continue
        k = np.arange(per[kind])
        slots = offs[kind] + (ce & 7)[:, None] * per[kind] + k[None, :]
        rows.append(e["s2h"][slots].ravel())
        cols.append(((ce >> 3)[:, None] + 0 * k[None, :]).ravel())
        dst.append(((soff[sg] + kbase[kind][sg] + sx * per[kind])[:, None] + k[None, :]).ravel())
        if gid.size == sg.size:                  # (ids every rank agrees on: a global analysis only)
            gids.append(((code << 40) + (gid[:, None] << 12) + k[None, :]).ravel())
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)
    members = [tuple(int(m) for m in smem[sptr[q]:sptr[q + 1]]) for q in range(nseg)]
    assert all(list(m) == sorted(set(m)) and g.rank in m for m in members) and len(set(members)) == nseg
    return {"rows": cat(rows), "cols": cat(cols), "dst": cat(dst), "gid": cat(gids), "members": members, "soff": soff, "size": size}


def segment_sums(layouts, bufs, descending=False):
    """Per rank the exchange buffer the segment form must end with: every segment the left-to-right float64 sum of its members'
    partial segments (bufs[m]: the buffer rank m sent) in ascending member rank -- or descending, for the condition on the
    inputs.  A segment is found on its other members by its member set; it has the same length and order there."""
    where = [{m: q for q, m in enumerate(lay["members"])} for lay in layouts]
    out = []
    for r, lay in enumerate(layouts):
        exp = np.full(int(lay["soff"][-1]), np.nan)
        for q, mem in enumerate(lay["members"]):
            acc = None
            for m in (reversed(mem) if descending else mem):
                qm = where[m][mem]
                assert layouts[m]["size"][qm] == lay["size"][q], (r, m, mem)
                o = int(layouts[m]["soff"][qm])
                v = bufs[m][o:o + int(lay["size"][q])]
                acc = v.copy() if acc is None else acc + v
            exp[int(lay["soff"][q]):int(lay["soff"][q + 1])] = acc
        out.append(exp)
    return out


def member_counts(layouts):
    """{number of members: doubles of this level in such segments, over all ranks}"""
    c = {}
    for lay in layouts:
        for mem, size in zip(lay["members"], lay["size"]):
            c[len(mem)] = c.get(len(mem), 0) + int(size)
    return c
