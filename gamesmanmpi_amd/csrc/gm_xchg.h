// gm_xchg.h -- the exchange layer the sharded host paths share (DENSE,
// PLANES, BUCKETED, RANKED): which transport a solve runs over and the group
// checks, an all-gather of a few u64 per rank, a ranged send / receive of
// device memory, and the end-of-solve reduction.  Host only, no kernels.
// Included by gm_solver.hip after struct gm_solver, before the layouts' host
// paths.  What a layout sends -- its ranges, fingerprints, packing kernels --
// stays in its own file.

// (gm_solver.hip includes this inside its extern "C" block: templates need
// C++ linkage)
extern "C++" {
// How the shards of a solve reach each other
enum Xchg : int {
  XCHG_TABLE = 0,    // one table, nothing to exchange
  XCHG_RCCL = 1,     // one shard per process (or per thread of solve_multi), RCCL
  XCHG_GROUP = 2,    // every shard in ss, on ONE stream: device copies in order
  XCHG_HOST = 3,     // one shard per process, the host-staged transport (s->xfer)
  XCHG_STREAMS = 4,  // every shard in ss, each on its own stream: the one-GPU rehearsal of XCHG_RCCL
};
static bool xchg_group(Xchg m) { return m == XCHG_GROUP || m == XCHG_STREAMS; }

// The mode of a solve over the shards ss of layout `layout` (GM_MODE_*), and
// the checks every layout makes: an RCCL shard has its communicator; a group
// holds all `world` shards, of that layout, in rank order, on one stream or
// each on its own.  What a layout refuses beyond this it checks itself.
static int xchg_mode(const std::vector<gm_solver*>& ss, uint32_t layout, Xchg* mode) {
  gm_solver* s0 = ss[0];
  const int W = s0->world;
  const bool own_streams = ss.size() > 1 && ss[1]->stream != s0->stream;
  const Xchg m = *mode = W <= 1          ? XCHG_TABLE
                         : ss.size() != 1 ? (own_streams ? XCHG_STREAMS : XCHG_GROUP)
                         : s0->xfer       ? XCHG_HOST
                                          : XCHG_RCCL;
  if (m == XCHG_RCCL && !s0->comm) return fail(GM_EINVAL, "shard %d/%d has no communicator (gm_solver_comm_init)", s0->rank, W);
  if (!xchg_group(m)) return 0;
  if ((int)ss.size() != W) return fail(GM_EINVAL, "group solve needs all %d shards", W);
  for (size_t g = 0; g < ss.size(); g++) {
    if (ss[g]->rank != (int)g || ss[g]->mode != layout)
      return fail(GM_EINVAL, "group shards must be ranks 0..n-1 of one layout");
    for (size_t h = 0; h < g; h++)
      if ((m == XCHG_GROUP) != (ss[g]->stream == ss[h]->stream))
        return fail(GM_EINVAL, "group shards share one stream, or (the RCCL rehearsal) each has its own");
  }
  return 0;
}

// an in-process multi-GPU group aborted (solve_multi's abort_all): no RCCL
// call may use the aborted communicators
#define RCCL_LIVE(S)                                                                              \
  do {                                                                                            \
    if ((S)->gabort && (S)->gabort->load(std::memory_order_acquire))                              \
      return fail(GM_EHIP, "RCCL group aborted: a peer shard failed (shard %d/%d)", (S)->rank, (S)->world); \
  } while (0)

static int xfer_call(gm_solver* s, int op, const void* sb, u64 sn, int sp, void* rb, u64 rn, int rp) {
  const int rc = s->xfer(s->xfer_ctx, op, sb, sn, sp, rb, rn, rp);
  return rc ? fail(GM_EHIP, "transport callback failed (%d) on rank %d", rc, s->rank) : 0;
}
// host-staged copy of device ranges into / out of s->hstage
struct HostRange {
  void* dev;
  u64 bytes;
};
static int stage_out(gm_solver* s, const std::vector<HostRange>& rs, u64 at, hipStream_t cs) {
  for (const HostRange& r : rs) {
    HIPCHK(hipMemcpyAsync(s->hstage.data() + at, r.dev, r.bytes, hipMemcpyDeviceToHost, cs));
    at += r.bytes;
  }
  HIPCHK(hipStreamSynchronize(cs));
  return 0;
}
static int stage_in(gm_solver* s, const std::vector<HostRange>& rs, u64 at, hipStream_t cs) {
  for (const HostRange& r : rs) {
    HIPCHK(hipMemcpyAsync(r.dev, s->hstage.data() + at, r.bytes, hipMemcpyHostToDevice, cs));
    at += r.bytes;
  }
  HIPCHK(hipStreamSynchronize(cs));
  return 0;
}
static u64 ranges_bytes(const std::vector<HostRange>& rs) {
  u64 n = 0;
  for (const HostRange& r : rs) n += r.bytes;
  return n;
}
// one paired transfer through the host: send ranges `out` to rank sp, receive
// ranges `in` from rank rp
static int xfer_ranges(gm_solver* s, const std::vector<HostRange>& out, int sp, const std::vector<HostRange>& in, int rp,
                       hipStream_t cs) {
  const u64 ns = ranges_bytes(out), nr = ranges_bytes(in);
  if (s->hstage.size() < ns + nr) s->hstage.resize(ns + nr);
  int rc = stage_out(s, out, 0, cs);
  if (rc) return rc;
  rc = xfer_call(s, GM_XFER_SENDRECV, s->hstage.data(), ns, sp, s->hstage.data() + ns, nr, rp);
  if (rc) return rc;
  return stage_in(s, in, ns, cs);
}

// ---------------------------------------------------------------------------
// all-gather of m u64 per rank
// ---------------------------------------------------------------------------
// One shard's row `mine` to every rank, every rank's into all[world * m]
// (rank-major).  XCHG_HOST: one GM_XFER_ALLGATHER; XCHG_RCCL: through the
// staging buffer kept with the solver (xdev, grown on demand, freed with it).
static int xchg_allgather_one(gm_solver* s, Xchg mode, hipStream_t st, const u64* mine, size_t m, u64* all) {
  const size_t n = m * (size_t)s->world;
  if (mode == XCHG_HOST) return xfer_call(s, GM_XFER_ALLGATHER, mine, m * 8, -1, all, n * 8, -1);
  if (s->xdev_n < m + n) {
    if (s->xdev) (void)hipFree(s->xdev);
    s->xdev = nullptr;
    s->xdev_n = 0;
    HIPCHK(hipMalloc((void**)&s->xdev, (m + n) * 8));
    s->xdev_n = m + n;
  }
  u64* dev = s->xdev;
  RCCL_LIVE(s);
  HIPCHK(hipMemcpyAsync(dev, mine, m * 8, hipMemcpyHostToDevice, st));
  const ncclResult_t r = ncclAllGather(dev, dev + m, m, ncclUint64, s->comm, st);
  hipError_t e = hipMemcpyAsync(all, dev + m, n * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (r != ncclSuccess) return fail(GM_EHIP, "RCCL all-gather: %s", ncclGetErrorString(r));
  if (e != hipSuccess) return fail(GM_EHIP, "all-gather: %s", hipGetErrorString(e));
  return 0;
}
// row(s, out) writes shard s's m values: a group fills every shard's row on
// the host, one shard per process gathers the others' over its transport
template <class Row>
static int xchg_allgather(std::vector<gm_solver*>& ss, Xchg mode, hipStream_t st, size_t m, std::vector<u64>& all,
                          Row&& row) {
  all.assign(m * (size_t)ss[0]->world, 0);
  if (xchg_group(mode)) {
    for (gm_solver* s : ss) row(s, &all[m * (size_t)s->rank]);
    return 0;
  }
  std::vector<u64> mine(m);
  row(ss[0], mine.data());
  return xchg_allgather_one(ss[0], mode, st, mine.data(), m, all.data());
}

// ---------------------------------------------------------------------------
// ranged send / receive
// ---------------------------------------------------------------------------
// A shard's messages of one exchange, in order: out[i] goes to out[i].peer,
// in[i] comes from in[i].peer; the k-th range a shard sends to a peer lands
// in the k-th range that peer receives from it.  Ranges of 0 bytes move
// nothing.
struct XRange {
  int peer;
  void* dev;
  u64 bytes;
};
struct XLists {
  std::vector<XRange> out, in;
};
// one pairwise round of the host transport: send to rank `to` while
// receiving from rank `from`
struct XRound {
  int to, from;
};
// the all-to-all schedule: W - 1 rounds, round k pairs r -> r + k with r - k -> r
static std::vector<XRound> xchg_rounds(int rank, int W) {
  std::vector<XRound> r;
  for (int k = 1; k < W; k++) r.push_back({(rank + k) % W, (rank - k + W) % W});
  return r;
}

// One shard over its transport, on stream cs.  Ranges to / from the shard
// itself are device copies.  XCHG_RCCL: one grouped set of sends and
// receives, each peer's in list order.  XCHG_HOST: the given rounds, one
// paired transfer each (a round with nothing to move still pairs up: its
// peer counts on the call).  `what` names the exchange in an RCCL error.
static int xchg_ranges(gm_solver* s, Xchg mode, hipStream_t cs, const XLists& x, const std::vector<XRound>& rounds,
                       const char* what) {
  {
    size_t i = 0;  // the shard's own ranges pair up in order
    for (const XRange& o : x.out) {
      if (o.peer != s->rank) continue;
      while (i < x.in.size() && x.in[i].peer != s->rank) i++;
      if (i == x.in.size() || x.in[i].bytes != o.bytes) return fail(GM_ECORRUPT, "exchange: self counts differ");
      if (o.bytes) HIPCHK(hipMemcpyAsync(x.in[i].dev, o.dev, o.bytes, hipMemcpyDeviceToDevice, cs));
      i++;
    }
  }
  if (mode == XCHG_RCCL) {
    RCCL_LIVE(s);
    ncclResult_t r = ncclGroupStart();
    for (const XRange& o : x.out)
      if (o.bytes && o.peer != s->rank && r == ncclSuccess) r = ncclSend(o.dev, o.bytes, ncclUint8, o.peer, s->comm, cs);
    for (const XRange& i : x.in)
      if (i.bytes && i.peer != s->rank && r == ncclSuccess) r = ncclRecv(i.dev, i.bytes, ncclUint8, i.peer, s->comm, cs);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return fail(GM_EHIP, "RCCL %s: %s", what, ncclGetErrorString(r != ncclSuccess ? r : r2));
    return 0;
  }
  for (const XRound& k : rounds) {
    std::vector<HostRange> out, in;
    for (const XRange& o : x.out)
      if (o.bytes && o.peer == k.to) out.push_back({o.dev, o.bytes});
    for (const XRange& i : x.in)
      if (i.bytes && i.peer == k.from) in.push_back({i.dev, i.bytes});
    int rc = xfer_ranges(s, out, k.to, in, k.from, cs);
    if (rc) return rc;
  }
  return 0;
}

// Every shard of an in-process group (x[g]: shard g's lists): what each
// shard sends to each peer must be what that peer expects, range by range
// (under RCCL a receive of another size would wait forever), then device
// copies.  XCHG_GROUP: on the one stream st, in the senders' order.
// XCHG_STREAMS: RCCL's grouped send / receive on each rank's own stream,
// rehearsed -- every sender's data is final on its stream (pev[0]); each
// receiver's stream waits for its senders and copies its incoming ranges;
// every stream then waits for every receiver (pev[1]): a send completes only
// with the transfer, so no rank reuses its buffers early.
static int xchg_copies(std::vector<gm_solver*>& ss, Xchg mode, hipStream_t st, const std::vector<XLists>& x) {
  const size_t W = ss.size();
  struct Copy {
    size_t from, to;
    void* src;
    void* dst;
    u64 bytes;
  };
  std::vector<Copy> cp;
  std::vector<size_t> at(W * W, 0);  // [p * W + r]: the next of p's receives from r
  for (size_t r = 0; r < W; r++)
    for (const XRange& o : x[r].out) {
      const size_t p = (size_t)o.peer;
      const std::vector<XRange>& in = x[p].in;
      size_t& i = at[p * W + r];
      while (i < in.size() && in[i].peer != (int)r) i++;
      const u64 want = i < in.size() ? in[i].bytes : 0;
      if (want != o.bytes)
        return fail(GM_ECORRUPT, "exchange: shard %d sends %llu bytes to %d, which expects %llu", (int)r,
                    (unsigned long long)o.bytes, (int)p, (unsigned long long)want);
      if (i < in.size()) cp.push_back({r, p, o.dev, in[i++].dev, o.bytes});
    }
  for (size_t p = 0; p < W; p++)  // a receive nobody sends
    for (size_t r = 0; r < W; r++)
      for (size_t i = at[p * W + r]; i < x[p].in.size(); i++)
        if (x[p].in[i].peer == (int)r && x[p].in[i].bytes)
          return fail(GM_ECORRUPT, "exchange: shard %d sends %llu bytes to %d, which expects %llu", (int)r, 0ull, (int)p,
                      (unsigned long long)x[p].in[i].bytes);
  if (mode == XCHG_GROUP) {
    for (const Copy& c : cp)
      if (c.bytes) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  for (gm_solver* s : ss)
    while (s->pev.size() < 2) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      s->pev.push_back(e);
    }
  for (gm_solver* s : ss) HIPCHK(hipEventRecord(s->pev[0], s->stream));
  for (size_t p = 0; p < W; p++) {
    gm_solver* t = ss[p];
    for (const Copy& c : cp) {  // (cp is sender-major: ascending senders here)
      if (c.to != p || !c.bytes) continue;
      if (c.from != p) HIPCHK(hipStreamWaitEvent(t->stream, ss[c.from]->pev[0], 0));
      HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, t->stream));
    }
    HIPCHK(hipEventRecord(t->pev[1], t->stream));
  }
  for (gm_solver* s : ss)
    for (gm_solver* t : ss)
      if (t != s) HIPCHK(hipStreamWaitEvent(s->stream, t->pev[1], 0));
  return 0;
}

// ---------------------------------------------------------------------------
// the end-of-solve reduction of red[5]: positions, edges, primitives, root
// word + 1 (summed), error bits (OR-ed)
// ---------------------------------------------------------------------------
// XCHG_RCCL, enqueued on st after the shard's red[] is final: the counts and
// the root word summed in place, every rank's error mask gathered into errg
static int xchg_reduce_rccl(gm_solver* s, hipStream_t st) {
  RCCL_LIVE(s);
  ncclGroupStart();
  ncclResult_t r = ncclAllReduce(s->st->red, s->st->red, 4, ncclUint64, ncclSum, s->comm, st);
  ncclResult_t r2 = ncclAllGather(s->st->red + 4, s->errg, 1, ncclUint64, s->comm, st);
  ncclResult_t r3 = ncclGroupEnd();
  if (r != ncclSuccess || r2 != ncclSuccess || r3 != ncclSuccess)
    return fail(GM_EHIP, "RCCL allreduce: %s", ncclGetErrorString(r != ncclSuccess ? r : r2 != ncclSuccess ? r2 : r3));
  return 0;
}
// shard s's red[] as read back on the host, r, folded into the job's totals:
// XCHG_HOST gathers every rank's; RCCL has reduced the counts already and
// the gathered error masks are OR-ed here; a group's shards add up
static int xchg_reduce_fold(gm_solver* s, Xchg mode, const u64 r[5], u64 red[5]) {
  auto add = [&](const u64* v) {
    for (int i = 0; i < 5; i++) red[i] = (i == 4) ? (red[i] | v[i]) : red[i] + v[i];
  };
  if (mode == XCHG_HOST) {
    std::vector<u64> all((size_t)5 * s->world);
    int rc = xchg_allgather_one(s, mode, nullptr, r, 5, all.data());
    if (rc) return rc;
    for (int g = 0; g < s->world; g++) add(&all[(size_t)g * 5]);
    return 0;
  }
  u64 v[5] = {r[0], r[1], r[2], r[3], r[4]};
  if (mode == XCHG_RCCL) {
    std::vector<u64> e((size_t)s->world);
    HIPCHK(hipMemcpy(e.data(), s->errg, e.size() * sizeof(u64), hipMemcpyDeviceToHost));
    v[4] = 0;
    for (u64 x : e) v[4] |= x;
  }
  add(v);
  return 0;
}
}  // extern "C++"
