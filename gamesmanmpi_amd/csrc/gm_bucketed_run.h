// gm_bucketed_run.h -- host side of the BUCKETED layout (kernels:
// gm_bucketed.h): which games it serves, the plan's bounds and scratch map,
// the solver's buffer carving and the one-GPU solve loop.  No kernels.
// Included by gm_solver.hip before gm_bucketed_shard.h, whose md5-sharded
// levels share these helpers.

// (gm_solver.hip includes this inside its extern "C" block: templates need
// C++ linkage)
extern "C++" {
// ---- BUCKETED plan ---------------------------------------------------------
// keyed games whose every move advances one level (the tier is the number
// of pieces placed): the bucketed pipeline applies (gm_bucketed.h)
// every move advances one level, and remoteness < 256 (packed backward answers)
static bool bk_ok(const Desc* d) { return kind_facts(d->kind).bucketed && d->max_levels <= 256; }
// edges bound for a positions bound: the known counts where the board and
// bound match (known_board, gm_registry.h), else a branching factor above
// every known board's
static const KnownBoard* bk_known(const Desc* d) {
  const KnownBoard* k = known_board(d);
  return k && k->edges ? k : nullptr;
}
static u64 bk_edges_bound(const Desc* d, u64 P) {
  const KnownBoard* k = bk_known(d);
  if (k && P <= k->positions) return k->edges + 1024;
  const double r = kind_facts(d->kind).edge_ratio, ratio = r ? r : (double)d->L;  // (0: at most one move per column)
  return (u64)(ratio * (double)P) + 1024;
}
// out-edges of the P positions an md5 shard owns: the md5 partition spreads
// positions evenly and regardless of their move counts, so a shard's share of
// the edges is its share of the positions -- the board's known edge / position
// ratio (+2 %), else the per-kind ratio; not the whole board's edges, which
// sized every shard of toot 6x4 for the full 4.2e9 (4 shards: out of memory)
static u64 bk_shard_edges_bound(const Desc* d, u64 P) {
  const KnownBoard* k = bk_known(d);
  if (k && P < k->positions)
    return std::min<u64>(k->edges, (u64)((double)k->edges / (double)k->positions * (double)P * 1.02)) + 1024;
  return bk_edges_bound(d, P);
}
// in-edges of the widest level: a quarter of all edges (every known board
// is below a fifth; a level over it returns GM_EFULL and the host re-plans)
// (+5% and a run per partition: the count-free expand provisions each of the
// 256 coarse partitions a 1/256 share of it, k_bk_expand<OVER>)
static u64 bk_emax_bound(u64 E) { return std::min<u64>(E, std::max<u64>(E / 4, 1u << 20)) / 20 * 21 + (u64)kBkC * 4096; }
// bytes of the table buffer ahead of the staging, as bk_setup carves them:
// the words, then the in-edges' parents (u32) and child indices (u16) -- a
// second set on md5 shards -- each array padded so that the next one, and at
// last the 8-byte staging keys, start aligned
static u64 bk_fixed_bytes(u64 Pcap, u64 Ecap, int world) {
  const u64 edges = 4 * Ecap + ((2 * Ecap + 7) & ~7ull);
  return ((4 * Pcap + 7) & ~7ull) + (world > 1 ? 2 : 1) * edges;
}
struct BkScratch {
  size_t lv, pbase, bh, ph, boff, tot, cbase, ah, cur, ucnt, total, gc, meta, end;
};
static BkScratch bk_scratch(int T) {
  auto r = [](size_t b) { return (b + 255) / 256 * 256; };
  BkScratch x;
  size_t o = r(devstate_bytes(T));
  x.lv = o; o += r(sizeof(BkLevel) * (size_t)T);
  x.pbase = o; o += r((size_t)T * (kBkC + 1) * 4);
  x.bh = o; o += r((size_t)kBkExpandBlocks * kBkC * 4);
  x.ph = o; o += r((size_t)kBkExpandBlocks * kBkC * 4);
  x.boff = o; o += r((size_t)kBkExpandBlocks * kBkC * 4);
  x.tot = o; o += r(2 * kBkC * 4);
  x.cbase = o; o += r((kBkC + 1) * 4);
  const size_t NBmax = (size_t)kBkC << kBkMaxFineBits;
  x.ah = o; o += r((size_t)T * kBkC * kBkC * 4);  // per level: answers per (child partition, parent range)
  x.cur = o; o += r((kBkC + ((size_t)1 << (29 - kBkRangeBits)) + 1) * 4);  // B3 / B4 run cursors
  x.ucnt = o; o += r(NBmax * 4);
  x.total = o; o += r(2 * 8);
  x.gc = o; o += r((2 * kBkC + 4) * 4);  // k_bk_expand<OVER>: partition cursors, parent-range totals, overflow flag
  const size_t NRmax = (size_t)1 << (29 - kBkRangeBits);
  // per level: cst, fo, rfo (twice: md5 shards' local-dedup form keeps a second cst / fo per level)
  x.meta = o; o += r((size_t)T * 2 * (2 * (NBmax + 1) + NRmax + 1) * 4);
  x.end = o;
  return x;
}

// ---------------------------------------------------------------------------
// BUCKETED solve (gm_bucketed.h).  Steps as in the other layouts: forward
// step L (L < T - 1) builds level L + 1 from level L; backward step
// 2T - 1 - L resolves level L.  The host reads back two small arrays per
// forward level (partition sizes, then the level's unique count) to size
// the next launches and check capacities BEFORE any kernel writes past
// them; the backward pass is enqueued without host round trips.
// ---------------------------------------------------------------------------
static uint32_t bitlen64(u64 x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }
// parent-range geometry of a level of n positions (B3-B5): coarse ranges
// index >> pshift (< 256 of them), fine ranges index >> fb (<= 2^13 parents,
// <= 256 per coarse range)
static bool bk_ranges(u64 n, uint32_t* pshift, uint32_t* fb) {
  const uint32_t bl = bitlen64(n ? n - 1 : 0);
  *pshift = bl > 8 ? bl - 8 : 0;
  *fb = std::min<uint32_t>(*pshift, (uint32_t)kBkRangeBits);
  return *pshift - *fb <= (uint32_t)kBkMaxFineBits;
}
// the bucketed kernels' instantiation for a descriptor (fixed_kind: the
// compile-time toot boards where one exists)
// (kernels that never generate children -- k_bk_reduce, k_bks_ownbin -- take
// bk_dispatch_plain: the symmetric kinds differ in `children` alone)
template <class Fn>
static void bk_dispatch_plain(const Desc& d, Fn&& fn) {
  kind_dispatch<BucketedKinds>(fixed_kind(d), fn);
}
template <class Fn>
static void bk_dispatch(const Desc& d, Fn&& fn) {  // children as orbit representatives where asked (gm_sym.h)
  kind_dispatch_sym<BucketedKinds>(d, fixed_kind(d), fn);
}
#define BK_KIND_LAUNCH(KERNEL, GRID, BLOCK, S, ...)                                                      \
  bk_dispatch((S)->d, [&](auto kind_) {                                                                  \
    constexpr int K_ = decltype(kind_)::value;                                                           \
    hipLaunchKernelGGL(KERNEL<K_>, dim3(GRID), dim3(BLOCK), 0, (S)->stream, __VA_ARGS__);               \
  })
#define BK_KIND_LAUNCH_PLAIN(KERNEL, GRID, BLOCK, S, ...)                                                      \
  bk_dispatch_plain((S)->d, [&](auto kind_) {                                                                  \
    constexpr int K_ = decltype(kind_)::value;                                                           \
    hipLaunchKernelGGL(KERNEL<K_>, dim3(GRID), dim3(BLOCK), 0, (S)->stream, __VA_ARGS__);               \
  })

// parents per expand round for a mean branching avg: the round's children
// should fill about 3/4 of the 8192-record stage (whole waves, 256..4096)
static uint32_t bk_ppr(double avg) {
  const double p = 0.75 * kBkExpandCap / std::max(avg, 0.25);
  return (uint32_t)std::min<double>(4.0 * kBkExpandThreads, std::max<double>(256.0, std::floor(p / 64.0) * 64.0));
}

// What a BUCKETED solver adds to the common fields: its arrays carved out of
// the table buffer, its tables out of the scratch (bk_scratch)
static void bk_setup(gm_solver* s, const gm_buffers* buf) {
  const int world = s->world;
  char* t = (char*)buf->table;
  s->Pcap = buf->level_capacity;
  s->Ecap = buf->table_slots;
  // a shard of a world > 1 job also holds the md5 exchange buffers (24 B per staged record)
  // (world > 1 also: the local-dedup form's in-edges, another 6 B per edge)
  // (the padded sizes: with 4 Pcap + 6 Ecap the last staging array ended up
  // to 10 bytes past table_bytes when Pcap was odd or Ecap no multiple of 4)
  const u64 fixed = bk_fixed_bytes(s->Pcap, s->Ecap, world);
  s->Emax = std::min<u64>((buf->table_bytes > fixed ? buf->table_bytes - fixed : 0) / (world > 1 ? 48 : 24), 0xFFFFFFF0ull);
  s->bkK = (u64*)buf->levels;
  s->bkW = (uint32_t*)t;
  t += (4 * s->Pcap + 7) & ~7ull;
  s->REp = (uint32_t*)t;
  t += 4 * s->Ecap;
  s->REc = (uint16_t*)t;
  t += (2 * s->Ecap + 7) & ~7ull;
  if (world > 1) {
    s->REpl = (uint32_t*)t;
    t += 4 * s->Ecap;
    s->REcl = (uint16_t*)t;
    t += (2 * s->Ecap + 7) & ~7ull;
  }
  // staging: [S1k | S1p | S1f] (the count-free expand writes the first 13
  // Emax bytes of it in its chunked layout, BkChunked) then S2k
  s->S1k = (u64*)t;
  t += 8 * s->Emax;
  s->S1p = (uint32_t*)t;
  t += 4 * s->Emax;
  s->S1f = (uint8_t*)t;  // (4 Emax bytes of the plan; one is used)
  t += 4 * s->Emax;
  s->S2k = (u64*)t;
  t += 8 * s->Emax;
  if (world > 1) {  // md5 exchange: records sent / received (keys, refs; answers reuse the key arrays)
    s->XSk = (u64*)t;
    t += 8 * s->Emax;
    s->XSr = (uint32_t*)t;
    t += 4 * s->Emax;
    s->XRk = (u64*)t;
    t += 8 * s->Emax;
    s->XRr = (uint32_t*)t;
  }
  const BkScratch x = bk_scratch(s->d.max_levels);
  char* sc = (char*)buf->scratch;
  s->bkL = (BkLevel*)(sc + x.lv);
  s->pbase = (uint32_t*)(sc + x.pbase);
  s->bh = (uint32_t*)(sc + x.bh);
  s->ph = (uint32_t*)(sc + x.ph);
  s->boff = (uint32_t*)(sc + x.boff);
  s->tot = (uint32_t*)(sc + x.tot);
  s->cbase = (uint32_t*)(sc + x.cbase);
  s->bkcur = (uint32_t*)(sc + x.cur);
  s->bkah = (uint32_t*)(sc + x.ah);
  s->bkgc = (uint32_t*)(sc + x.gc);
  s->ucnt = (uint32_t*)(sc + x.ucnt);
  s->bktotal = (u64*)(sc + x.total);
  s->meta = (uint32_t*)(sc + x.meta);
  s->meta_cap = (x.end - x.meta) / 4;
}

static int solve_bucketed(gm_solver* s, gm_result* out) {
  const Desc& d = s->d;
  const int T = d.max_levels;
  const int first = (int)s->step_first, stop = s->step_stop ? (int)s->step_stop : 2 * T;
  s->step_first = s->step_stop = 0;
  const bool timing = (s->flags & GM_F_KERNEL_TIMING) && first == 0 && stop == 2 * T;
  hipStream_t st = s->stream;
  SolveEvents ev;
  if (ev.begin()) return GM_EHIP;
  const hipEvent_t e0 = ev.e0, e1 = ev.e1, e2 = ev.e2;
  // kernel-time spans (timing): [start, stop, forward?]
  struct Span {
    hipEvent_t a, b;
    bool fwd;
  };
  std::vector<Span> spans;
  u64 nfwd = 0, nbwd = 0;
  auto span = [&](bool fwd) -> hipEvent_t* {  // opens a span; returns its stop event to record later
    if (!timing) return nullptr;
    Span x{};
    x.fwd = fwd;
    if (ev.make(&x.a) || ev.make(&x.b)) return nullptr;
    if (hipEventRecord(x.a, st) != hipSuccess) return nullptr;
    spans.push_back(x);
    return &spans.back().b;
  };
  auto span_end = [&](hipEvent_t* b) -> int {
    if (b) HIPCHK(hipEventRecord(*b, st));
    return 0;
  };
  int rc = 0;
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(st);
    return code;
  };
  auto t0 = std::chrono::steady_clock::now();
  HIPCHK(hipEventRecord(e0, st));
  std::vector<BkLevel>& lv = s->lvh;
  if (first == 0) {
    HIPCHK(hipMemsetAsync(s->st, 0, devstate_bytes(T), st));
    HIPCHK(hipMemsetAsync(s->bkL, 0, sizeof(BkLevel) * (size_t)T, st));
    lv.assign((size_t)T, BkLevel{});
    lv[0].n = 1;
    HIPCHK(hipMemcpyAsync(s->bkK, &s->d.root, sizeof(u64), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->bkL, lv.data(), sizeof(BkLevel), hipMemcpyHostToDevice, st));
  } else {
    lv.assign((size_t)T, BkLevel{});
    HIPCHK(hipMemcpyAsync(lv.data(), s->bkL, sizeof(BkLevel) * (size_t)T, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  std::vector<uint32_t> htot(2 * kBkC);
  std::vector<std::vector<uint32_t>> keep;  // host arrays of async H2D copies, alive until the end
  uint32_t herr = 0;
  // ---- forward ----
  for (int L = first; L < T && L < stop; L++) {
    if (L + 1 >= T) continue;  // the last level expands nothing (backward checks it holds only primitives)
    BkLevel& P = lv[(size_t)L];
    BkLevel& X = lv[(size_t)L + 1];
    u64 re_used = P.rb + P.ein;
    u64 meta_used = 0;  // end of the meta tables of the levels so far
    for (int i = 0; i <= L; i++) {
      const BkLevel& Q = lv[(size_t)i];
      if (Q.nbits) meta_used = std::max<u64>(meta_used, Q.cst_off + 2 * ((1ull << Q.nbits) + 1));
      if (i < L && Q.eout) meta_used = std::max<u64>(meta_used, Q.rfo_off + ((Q.n + (1ull << Q.fb) - 1) >> Q.fb) + 1);
    }
    X = BkLevel{};
    X.lb = P.lb + P.n;
    X.rb = re_used;
    if (!bk_ranges(P.n, &P.pshift, &P.fb))
      return bail(fail(GM_ELIMIT, "level %d holds %llu positions: more than the 2^29 a bucketed level supports", L,
                       (unsigned long long)P.n));
    P.eout = 0;
    if (P.n) {
      const u64 nblk = std::min<u64>(kBkExpandBlocks, (P.n + kBkExpandThreads - 1) / kBkExpandThreads),
                chunk = (P.n + nblk - 1) / nblk;
      const uint32_t NR = (uint32_t)((P.n + (1ull << P.fb) - 1) >> P.fb);
      if (meta_used + NR + 1 > s->meta_cap) return bail(fail(GM_ECORRUPT, "bucket tables exceed the scratch"));
      P.rfo_off = (uint32_t)meta_used;
      meta_used += NR + 1;
      uint32_t* rfo = s->meta + P.rfo_off;  // answers per fine parent range -> their starts
      keep.emplace_back(2 * (kBkC + 1));
      std::vector<uint32_t>& hb = keep.back();  // [coarse bases | parent-range bases]
      u64 E = 0, Ep = 0;
      // Count-free form first (k_bk_expand<OVER>): children go straight to
      // provisioned partitions; a partition past its share -> the exact
      // form (F0 counts, then k_bk_expand<false>) for this level.
      // a partition's provisioned share, whole chunks of the chunked staging
      uint32_t ck_sh = 14;
      while (ck_sh > 6 && (s->Emax / kBkC) < (1ull << ck_sh)) ck_sh--;
      const uint32_t cap = (uint32_t)((s->Emax / kBkC) >> ck_sh << ck_sh);
      const BkChunked ck{(char*)s->S1k, ck_sh};
      uint32_t incap = 0;
      bool exact = true;
      hipEvent_t* sp = nullptr;
      if (!(s->flags & GM_F_BK_EXACT)) {
        HIPCHK(hipMemsetAsync(rfo, 0, (NR + 1) * 4, st));
        HIPCHK(hipMemsetAsync(s->bkgc, 0, (2 * kBkC + 4) * 4, st));
        // parents per round from the previous level's branching (a round's
        // children should fill most of the 8192-record stage)
        const double avg = (L > 0 && lv[(size_t)L - 1].n) ? std::max(1.0, (double)P.ein / (double)lv[(size_t)L - 1].n) : 4.0;
        const uint32_t ppr = bk_ppr(avg);
        sp = span(true);
        bk_dispatch(s->d, [&](auto kind_) {
          constexpr int K_ = decltype(kind_)::value;
          hipLaunchKernelGGL((k_bk_expand<K_, true>), dim3(nblk), dim3(kBkExpandThreads), 0, st, s->d, s->bkK + P.lb, P.n,
                             chunk, (const uint32_t*)nullptr, (const uint32_t*)nullptr, ppr, s->S1k, s->S1p, s->S1f, cap,
                             s->bkgc, P.pshift, P.fb, s->bkgc + kBkC, rfo, s->bkgc + 2 * kBkC, s->st, ck);
        });
        hipLaunchKernelGGL(k_bk_scan, dim3(1), dim3(1024), 0, st, rfo, NR + 1, rfo, s->bktotal + 1);
        if ((rc = span_end(sp))) return bail(rc);
        nfwd += 2;
        HIPCHK(hipGetLastError());
        std::vector<uint32_t> g(2 * kBkC + 1);
        HIPCHK(hipMemcpyAsync(g.data(), s->bkgc, g.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&herr, &s->st->err, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (herr) return bail(fail(GM_ECORRUPT, "level %d:%s", L, err_text(herr).c_str()));
        if (!g[2 * kBkC]) {
          exact = false;
          incap = cap;
          for (int j = 0; j < kBkC; j++) {
            hb[(size_t)j] = (uint32_t)E;
            hb[(size_t)kBkC + 1 + j] = (uint32_t)Ep;
            E += g[(size_t)j];
            Ep += g[(size_t)kBkC + j];
          }
        }
      }
      if (exact) {
        HIPCHK(hipMemsetAsync(rfo, 0, (NR + 1) * 4, st));
        sp = span(true);
        BK_KIND_LAUNCH(k_bk_count, nblk, kBkStreamThreads, s, s->d, s->bkK + P.lb, P.n, chunk, P.pshift, P.fb, s->bh,
                       s->ph, rfo, s->st);
        hipLaunchKernelGGL(k_bk_colscan, dim3(kBkC), dim3(256), 0, st, s->bh, (uint32_t)nblk, s->boff, s->tot);
        hipLaunchKernelGGL(k_bk_colscan, dim3(kBkC), dim3(256), 0, st, s->ph, (uint32_t)nblk, s->ph, s->tot + kBkC);
        hipLaunchKernelGGL(k_bk_scan, dim3(1), dim3(1024), 0, st, rfo, NR + 1, rfo, s->bktotal + 1);
        if ((rc = span_end(sp))) return bail(rc);
        nfwd += 4;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(htot.data(), s->tot, 2 * kBkC * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&herr, &s->st->err, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (herr) return bail(fail(GM_ECORRUPT, "level %d:%s", L, err_text(herr).c_str()));
        for (int j = 0; j < kBkC; j++) {
          hb[(size_t)j] = (uint32_t)E;
          hb[(size_t)kBkC + 1 + j] = (uint32_t)Ep;
          E += htot[(size_t)j];
          Ep += htot[(size_t)kBkC + j];
        }
      }
      if (E != Ep) return bail(fail(GM_ECORRUPT, "level %d: %llu children by partition, %llu by parent", L,
                                    (unsigned long long)E, (unsigned long long)Ep));
      if (E > s->Emax) return bail(fail(GM_EFULL, "level %d emits %llu children; the plan holds %llu per level", L,
                                        (unsigned long long)E, (unsigned long long)s->Emax));
      if (re_used + E > s->Ecap) return bail(fail(GM_EFULL, "edges exceed the plan's %llu", (unsigned long long)s->Ecap));
      hb[(size_t)kBkC] = (uint32_t)E;
      hb[(size_t)2 * kBkC + 1] = (uint32_t)Ep;
      P.eout = E;
      X.ein = E;
      HIPCHK(hipMemcpyAsync(s->cbase, hb.data(), (kBkC + 1) * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(s->pbase + (size_t)L * (kBkC + 1), hb.data() + kBkC + 1, (kBkC + 1) * 4,
                            hipMemcpyHostToDevice, st));
      if (E) {
        uint32_t f = 0;
        while (f < (uint32_t)kBkMaxFineBits && (E >> f) > (u64)kBkC * 4096) f++;
        const uint32_t F = 1u << f, NB = (uint32_t)kBkC << f;
        X.nbits = 8 + f;
        if (meta_used + 2 * (NB + 1) > s->meta_cap) return bail(fail(GM_ECORRUPT, "bucket tables exceed the scratch"));
        X.cst_off = (uint32_t)meta_used;
        uint32_t* cst = s->meta + X.cst_off;
        uint32_t* fo = cst + NB + 1;  // kept: the backward pass walks the level's in-edges bucket by bucket
        const int gd = (int)std::min<uint32_t>(NB, 512);  // two workgroups per CU
        sp = span(true);
        if (exact) {  // parents per expand round: about a stage (8192 records) of children
          const double avg = (double)E / (double)P.n;
          const uint32_t ppr = bk_ppr(avg);
          bk_dispatch(s->d, [&](auto kind_) {
            constexpr int K_ = decltype(kind_)::value;
            hipLaunchKernelGGL((k_bk_expand<K_, false>), dim3(nblk), dim3(kBkExpandThreads), 0, st, s->d, s->bkK + P.lb,
                               P.n, chunk, (const uint32_t*)s->boff, (const uint32_t*)s->cbase, ppr, s->S1k, s->S1p,
                               s->S1f, 0u, (uint32_t*)nullptr, 0u, 0u, (uint32_t*)nullptr, (uint32_t*)nullptr,
                               (uint32_t*)nullptr, s->st, BkChunked{nullptr, 0});
          });
          nfwd++;
        }
        // the fine partition writes the parents straight into the level's
        // in-edge parents (REp); F3 adds the child indices (REc)
        hipLaunchKernelGGL(k_bk_fine, dim3(kBkC), dim3(kBkFineThreads), 0, st, (const u64*)s->S1k,
                           (const uint32_t*)s->S1p, (const uint8_t*)s->S1f, (const uint32_t*)s->cbase, 8u - f, F, s->S2k,
                           s->REp + X.rb, fo, P.pshift, s->bkah + (size_t)L * kBkC * kBkC, incap, ck);
        // unique keys of bucket b to S1k[fo[b] ..), compacted into the level
        hipLaunchKernelGGL(k_bk_dedup, dim3(gd), dim3(kBkDedupThreads), 0, st, s->S2k, (const uint32_t*)fo, NB, s->S1k,
                           s->ucnt, s->REc + X.rb, s->st);
        hipLaunchKernelGGL(k_bk_scan, dim3(1), dim3(1024), 0, st, s->ucnt, NB, cst, s->bktotal);
        if ((rc = span_end(sp))) return bail(rc);
        nfwd += 3;
        HIPCHK(hipGetLastError());
        u64 n1 = 0;
        HIPCHK(hipMemcpyAsync(&n1, s->bktotal, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&herr, &s->st->err, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (herr) {
          // a fine bucket over kBkMaxUnique keys follows from the level's
          // real edges, not from the buffers: more memory cannot fix it
          const bool lim = herr & ERR_BUCKET_FULL;
          return bail(fail(lim ? GM_ELIMIT : GM_ECORRUPT, "level %d:%s", L + 1, err_text(herr).c_str()));
        }
        if (X.lb + n1 > s->Pcap) return bail(fail(GM_EFULL, "positions exceed the plan's %llu", (unsigned long long)s->Pcap));
        X.n = n1;
        sp = span(true);
        hipLaunchKernelGGL(k_bk_compact, dim3(std::min<uint32_t>(NB, 4096)), dim3(256), 0, st, (const u64*)s->S1k,
                           (const uint32_t*)fo, (const uint32_t*)cst, NB, s->bkK + X.lb);
        if ((rc = span_end(sp))) return bail(rc);
        nfwd++;
        HIPCHK(hipGetLastError());
      }
    }
    HIPCHK(hipMemcpyAsync(s->bkL + L, &lv[(size_t)L], 2 * sizeof(BkLevel), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(e1, st));
  // ---- backward ----
  for (int L = T - 1; L >= 0; L--) {
    const int k = 2 * T - 1 - L;
    if (k < first) continue;
    if (k >= stop) break;
    BkLevel& P = lv[(size_t)L];
    if (!P.n) continue;
    if (!bk_ranges(P.n, &P.pshift, &P.fb)) return bail(fail(GM_ELIMIT, "level %d too wide for bucketed levels", L));
    const uint32_t NR = (uint32_t)((P.n + (1ull << P.fb) - 1) >> P.fb);
    const int gr = (int)std::min<uint32_t>(NR, 512);
    hipEvent_t* sp = span(false);
    if (L + 1 < T && P.eout) {
      const BkLevel& X = lv[(size_t)L + 1];
      const uint32_t NB = 1u << X.nbits, F = NB / kBkC;
      const uint32_t* cst = s->meta + X.cst_off;
      const uint32_t* fo = cst + NB + 1;
      const uint32_t* rfo = s->meta + P.rfo_off;
      const uint32_t* pb = s->pbase + (size_t)L * (kBkC + 1);
      uint32_t* Ap = (uint32_t*)s->S1k;
      constexpr uint32_t K = kBkSplitK;  // B4 workgroups per range
      // B3: one workgroup per children's partition, exact offsets per
      // (partition, parent range) from the counts F2 kept (ah).  (Measured:
      // K = 4 workgroups of 512 threads per partition on device run cursors
      // took 50.5 ms of backward against 48.2 for this form.)
      hipLaunchKernelGGL(k_bk_colscan, dim3(kBkC), dim3(256), 0, st, s->bkah + (size_t)L * kBkC * kBkC, (uint32_t)kBkC,
                         s->boff, s->tot);
      hipLaunchKernelGGL(k_bk_answer, dim3(kBkC), dim3(kBkStreamThreads), 0, st, s->REp + X.rb, s->REc + X.rb, fo, cst,
                         NB, F, P.pshift, s->boff, pb, s->bkW + X.lb, Ap, s->st);
      nbwd += 2;
      const uint32_t Fp = 1u << (P.pshift - P.fb);
      const uint32_t* ap = Ap;
      if (Fp > 1) {
        HIPCHK(hipMemcpyAsync(s->bkcur + kBkC, rfo, (size_t)NR * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_bk_split, dim3(kBkC * K), dim3(kBkStreamThreads), 0, st, (const uint32_t*)Ap, pb,
                           10u + P.fb, Fp, K, s->bkcur + kBkC, (uint32_t*)s->S2k);
        ap = (uint32_t*)s->S2k;
        nbwd++;
      }
      BK_KIND_LAUNCH_PLAIN(k_bk_reduce, gr, kBkReduceThreads, s, s->d, s->bkK + P.lb, P.n, ap, rfo, P.fb, Fp - 1, NR,
                     s->bkW + P.lb, s->st);
    } else {
      BK_KIND_LAUNCH_PLAIN(k_bk_reduce, gr, kBkReduceThreads, s, s->d, s->bkK + P.lb, P.n, (const uint32_t*)nullptr,
                     (const uint32_t*)nullptr, P.fb, 0u, NR, s->bkW + P.lb, s->st);
    }
    nbwd++;
    if ((rc = span_end(sp))) return bail(rc);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(e2, st));
  if (stop < 2 * T) {  // stopped early: the state stays in the buffers for a resume
    HIPCHK(hipMemcpyAsync(s->bkL, lv.data(), sizeof(BkLevel) * (size_t)T, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GM_PARTIAL;
  }
  HIPCHK(hipMemcpyAsync(s->bkL, lv.data(), sizeof(BkLevel) * (size_t)T, hipMemcpyHostToDevice, st));
  uint32_t root_word = NO_WORD;
  HIPCHK(hipMemcpyAsync(&root_word, s->bkW, 4, hipMemcpyDeviceToHost, st));
  std::vector<unsigned char> host(devstate_bytes(T));
  HIPCHK(hipMemcpyAsync(host.data(), s->st, host.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  auto t1 = std::chrono::steady_clock::now();
  const DevState* hs = (const DevState*)host.data();
  float f = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&f, e0, e1));
  HIPCHK(hipEventElapsedTime(&b, e1, e2));
  out->ms_forward = f;
  out->ms_backward = b;
  out->ms_total = std::chrono::duration<double, std::milli>(t1 - t0).count();
  if (timing) {
    double sx = 0, sr = 0;
    for (const Span& x : spans) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, x.a, x.b));
      (x.fwd ? sx : sr) += ms;
    }
    out->ms_expand_kernels = sx;
    out->ms_resolve_kernels = sr;
    out->n_expand_launches = nfwd;
    out->n_resolve_launches = nbwd;
  }
  u64 pos = 0, wmax = 0;
  uint32_t nlev = 0;
  for (const BkLevel& x : lv) {
    pos += x.n;
    wmax = std::max<u64>(wmax, x.n);
    nlev += x.n > 0;
  }
  out->positions = pos;
  out->edges = hs->edges;
  out->primitives = hs->prims;
  out->levels = nlev;
  out->max_level_width = (uint32_t)std::min<u64>(wmax, 0xFFFFFFFFull);
  out->root_word = root_word;
  if (hs->err) {
    const bool full = hs->err & (ERR_TABLE_FULL | ERR_LEVELS_FULL);
    const bool lim = hs->err & ERR_BUCKET_FULL;
    return fail(lim ? GM_ELIMIT : full ? GM_EFULL : GM_ECORRUPT, "solve failed:%s", err_text(hs->err).c_str());
  }
  if (root_word == NO_WORD) return fail(GM_ECORRUPT, "root unresolved");
  out->root_value = (int32_t)(root_word & 3u);
  out->root_remoteness = root_word >> 2;
  return 0;
}
}  // extern "C++"
