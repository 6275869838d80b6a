// gm_dense_run.h -- host side of the DENSE layout (kernels: gm_dense.h): the
// solver's setup and kernel families, the per-level launches, the halo
// exchanges of a shard group with their fail-fast plan check, the solve loop
// (run_dense: one table, an in-process shard group, or one shard per process
// over RCCL / a host-staged transport) and the plan.  No kernels.  Included
// by gm_solver.hip after the solver object, k_fill_red and the shards'
// exchange layer (gm_xchg.h).

// (gm_solver.hip includes this inside its extern "C" block: templates need
// C++ linkage)
extern "C++" {
// ---------------------------------------------------------------------------
// setup: the tables a solver is created with
// ---------------------------------------------------------------------------
// Per-lane condition masks of a 64-prefix group for power-of-two layouts
// (k_dense_pull_words): with j the lane's offset in the group,
//   M[t]              = { j : sum_i digit_i(j) <= t }   (TS)
//   M[64 (i + 1) + t] = { j : digit_i(j) <= t }         (TD[i], i >= 1)
// They depend only on the descriptor, so they are built once here.
static void build_mask_tables(const Desc& d, u64* M) {
  memset(M, 0, kMaskTableWords * sizeof(u64));
  for (int j = 0; j < 64; j++) {
    uint32_t dj[16] = {0}, sj = 0;
    for (int i = 1; i < d.nheaps; i++) {
      dj[i] = (uint32_t)((j >> d.pshift[i]) & (d.base[i] - 1));
      sj += dj[i];
    }
    for (int t = 0; t < 64; t++) {
      if (sj <= (uint32_t)t) M[t] |= 1ull << j;
      for (int i = 1; i < d.nheaps; i++)
        if (dj[i] <= (uint32_t)t) M[64 * (i + 1) + t] |= 1ull << j;
    }
  }
}

// Column tables of the packed halos (k_halo_cols).  Slot j of a column
// (j < 256, digit sum ds(j) over the digits below the top) is a non-hole of
// slice x iff ds(j) in [y - heap0, y], y = x - gs: NY[y] counts them,
// PB[x][g] sums NY over the columns of smaller sum, and tot[x] = PB[x][NG-1]
// is the slice's non-hole total.
static void build_halo_cols(const Desc& d, const HaloGeom& h, const std::vector<uint32_t>& cstart,
                            std::vector<uint32_t>& PB, std::vector<uint32_t>& NY, std::vector<uint32_t>& CS,
                            std::vector<uint32_t>& tot) {
  const int H0 = (int)d.heap[0];
  NY.assign((size_t)h.NYn, 0);
  for (int j = 0; j < 256; j++) {
    int ds = 0;
    for (int i = 1; i < h.top; i++) ds += (int)(((uint32_t)j >> d.pshift[i]) & (d.base[i] - 1));
    for (int y = ds; y <= ds + H0 && y < h.NYn; y++) NY[(size_t)y]++;
  }
  CS.assign((size_t)h.NG, 0);
  std::vector<uint32_t> cnt((size_t)h.NG, 0);
  for (int g = 0; g < h.NG; g++) {
    CS[(size_t)g] = g + 1 < (int)cstart.size() ? cstart[(size_t)g] : cstart.back();
    if (g + 1 < (int)cstart.size()) cnt[(size_t)g] = cstart[(size_t)g + 1] - cstart[(size_t)g];
  }
  PB.assign((size_t)h.XN * h.NG, 0);
  tot.assign((size_t)h.XN, 0);
  for (int x = 0; x < h.XN; x++) {
    uint32_t run = 0;
    for (int g = 0; g < h.NG; g++) {
      PB[(size_t)x * h.NG + g] = run;
      const int y = x - g;
      if (y >= 0 && y < h.NYn) run += cnt[(size_t)g] * NY[(size_t)y];
    }
    tot[(size_t)x] = run;
  }
}

// local slice index of slice o of local block j
static u64 blk_slice(const gm_solver* s, u64 j, u64 o) { return j * (s->view.B + 4) + o; }
// global top value of slice o of local block j
static int64_t blk_top(const gm_solver* s, u64 j, u64 o) {
  return (int64_t)(((u64)s->view.rank + j * s->view.world) * s->view.B + o) - 2;
}
static u64 blk_count(const gm_solver* s) { return s->view.Wl / ((s->view.B + 4) * s->view.Z); }
static u64 blk_global(const gm_solver* s, u64 j) { return (u64)s->view.rank + j * s->view.world; }

// Kernel families of a dense solver (DenseResolveKind / DensePullKind),
// chosen once from the descriptor, the geometry, the scratch the caller
// provided and the flags.  16-bit tables: world 1 needs the live-group
// lists (octets sweep only listed groups); shards need the column
// permutation, packed 16-bit halos and every level's slices in one job list.
static int dense_choose(gm_solver* s) {
  const Desc& d = s->d;
  const DenseView& v = s->view;
  s->pk = d.pow2 ? PK_WORDS : PK_LANE;
  const bool scalar = (s->flags & GM_F_RESOLVE_SCALAR) != 0;
  const bool quad = d.pow2 && d.nheaps >= 2 && d.base[1] >= 4 && v.Wl * 4 <= 0xFFFFFFF0ull && (!v.blk || v.Z % 256 == 0);
  const bool base16 = d.pow2 && d.kind == K_SUM && d.nheaps >= 2 && d.nheaps <= 8 && d.base[1] >= 8 &&
                      d.root_sum < 0x7FFF && v.Wl * 2 <= 0xFFFFFFF0ull &&
                      !(s->flags & (GM_F_WORDS32 | GM_F_RESOLVE_SCALAR));
  s->w8 = false;
  if (!v.blk) {
    if (s->plan_bits < 32) {
      if (!s->glist)
        return fail(GM_EINVAL, "%u-bit dense table without live-group lists: scratch smaller than gm_plan's",
                    s->plan_bits);
      s->w16 = s->plan_bits == 16;
      s->w8 = s->plan_bits == 8;
      s->rk = s->w8 ? RK_HEX_LIST : RK_OCT_LIST;
      return 0;
    }
    s->w16 = false;
    s->rk = (scalar || !quad) ? RK_SCALAR : s->glist ? RK_QUAD_LIST : RK_QUAD_BAND;
    return 0;
  }
  s->w16 = base16 && d.nheaps >= 3 && s->colperm && s->hg.on && s->halo16 && v.Z % 256 == 0 && v.E <= 0xFFFF &&
           blk_count(s) * (v.B + 4) <= (u64)kMaxColJobs;
  s->rk = s->w16 ? RK_OCT_COLS : (scalar || !quad) ? RK_SCALAR : s->colperm ? RK_QUAD_COLS : RK_QUAD_BAND;
  return 0;
}

// The device-free half of a dense solver's geometry, written once: a solver
// (dense_setup) and the GPU-less exchange-plan signatures (shard_host_geom)
// both build it here, so the plan that is signed is the plan that runs.
// Fills s->cstart, s->hg, s->halo_tot and s->halo16 of a power-of-two table
// and returns the tables dense_setup uploads.
struct DenseHostGeom {
  ColGeom cg;
  bool perm_ok = false;  // a column permutation exists and the scratch has room for it
  size_t hbytes = 0;     // scratch the plan gives the halo tables and buffers
  std::vector<uint32_t> perm, PB, NY, CS;
};
// `room`: scratch bytes past the fixed part (scratch_bytes_for).  The solver
// reads the column permutation on the device, so packed halos need it to
// fit: scratch from an older plan (no room) falls back to whole-slice halos.
// gm_shard_halo_sigs has no scratch and needs only cg.on: it passes SIZE_MAX
// and signs the plan of a solver made from gm_plan_shard's scratch.
static DenseHostGeom dense_host_geom(gm_solver* s, size_t room) {
  const Desc* d = &s->d;
  DenseHostGeom h;
  h.cg = col_geom(d);
  if (h.cg.on) build_colperm(d, h.cg, h.perm, s->cstart);
  s->hg = halo_geom(d, s->world, s->view.blk ? blk_count(s) : 1);
  h.hbytes = s->hg.on ? halo_bytes(s->hg) : 0;
  h.perm_ok = h.cg.on && room >= h.hbytes + col_bytes(d);
  if (s->hg.on && h.perm_ok) {
    build_halo_cols(*d, s->hg, s->cstart, h.PB, h.NY, h.CS, s->halo_tot);
    s->halo16 = d->kind == K_SUM && d->root_sum < 32768;
  } else {
    s->hg.on = false;
  }
  return h;
}

// host half of a dense shard's halo geometry, as dense_setup builds it from a
// gm_plan_shard scratch (column permutation present)
static int shard_host_geom(const Desc* d, int rank, int world, gm_solver* s) {
  DenseGeom g;
  memset(&g, 0, sizeof g);
  int rc = dense_geom(d, rank, world, &g);
  if (rc) return rc;
  s->d = *d;
  s->mode = GM_MODE_DENSE;
  s->view = g.v;
  s->rank = rank;
  s->world = world;
  s->nblocks = g.nblocks;
  s->hg.on = false;
  if (d->pow2) dense_host_geom(s, SIZE_MAX);
  return 0;
}

// The live-group lists of every level (GroupGeom, gm_solver.hip: the order
// and its reasons): fills s->goff and s->gxcd and returns the entries.  Per
// level, 8 contiguous column ranges of ~equal live count, one per XCD, each
// walked top-major.
static std::vector<uint32_t> dense_group_lists(gm_solver* s, const GroupGeom& gg, size_t reserve) {
  const Desc* d = &s->d;
  std::vector<uint16_t> gsum;
  group_sums(d, gg, gsum);
  std::vector<uint32_t> list;
  list.reserve(reserve);
  s->goff.assign((size_t)d->max_levels + 1, 0);
  s->gxcd.assign((size_t)d->max_levels * 9, 0);
  const int top = d->nheaps - 1;
  const u64 C = d->pstride[top] / 256;  // groups per top-digit slice
  const bool cols = top >= 2 && d->pstride[top] % 256 == 0 && C >= 8;
  const u64 NT = cols ? gg.groups / C : 1, NC = cols ? C : gg.groups;
  std::vector<u64> live(NC);
  for (int L = 0; L < d->max_levels; L++) {
    s->goff[L] = list.size();
    u64 tot = 0;
    for (u64 c = 0; c < NC; c++) {
      u64 n = 0;
      for (u64 t = 0; t < NT; t++) n += group_live(d, gg, gsum[c + t * NC], L);
      live[c] = n;
      tot += n;
    }
    u64 c0 = 0, acc = 0;
    for (int x = 0; x < 8; x++) {
      s->gxcd[(size_t)L * 9 + x] = (uint32_t)(list.size() - s->goff[L]);
      u64 c1 = c0;
      const u64 want = tot * (u64)(x + 1) / 8;
      while (c1 < NC && (acc < want || x == 7)) acc += live[c1++];
      for (u64 t = 0; t < NT; t++)
        for (u64 c = c0; c < c1; c++)
          if (group_live(d, gg, gsum[c + t * NC], L)) list.push_back((uint32_t)(c + t * NC));
      c0 = c1;
    }
    s->gxcd[(size_t)L * 9 + 8] = (uint32_t)(list.size() - s->goff[L]);
  }
  s->goff[d->max_levels] = list.size();
  return list;
}

// What a DENSE solver adds to the common fields: the mask tables, the host
// geometry's tables where the scratch has room, the live-group lists, and the
// kernel families.  Scratch past the fixed part:
// [halo tables + buffers | column permutation | group lists]
static int dense_setup(gm_solver* s, const gm_buffers* buf) {
  const Desc* d = &s->d;
  if (d->pow2) {
    auto upload = [](void* dst, const void* src, size_t bytes) {
      return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    std::vector<u64> m(kMaskTableWords);
    build_mask_tables(*d, m.data());
    hipError_t e = upload((void*)s->masks, m.data(), m.size() * sizeof(u64));
    if (e != hipSuccess) return fail(GM_EHIP, "mask tables: %s", hipGetErrorString(e));
    size_t off = scratch_bytes_for(d->max_levels);
    const DenseHostGeom h = dense_host_geom(s, buf->scratch_bytes - off);
    if (h.perm_ok) {
      uint32_t* dp = (uint32_t*)((char*)buf->scratch + off + h.hbytes);
      e = upload(dp, h.perm.data(), h.perm.size() * 4);
      if (e != hipSuccess) return fail(GM_EHIP, "column permutation: %s", hipGetErrorString(e));
      s->colperm = dp;
      s->cg = h.cg;
    }
    if (s->hg.on) {
      char* base = (char*)buf->scratch + off;
      auto r = [](size_t b) { return (b + 255) / 256 * 256; };
      uint32_t* pb = (uint32_t*)base;
      uint32_t* ny = (uint32_t*)(base + r(h.PB.size() * 4));
      uint32_t* cs = (uint32_t*)(base + r(h.PB.size() * 4) + r(h.NY.size() * 4));
      e = upload(pb, h.PB.data(), h.PB.size() * 4);
      if (e == hipSuccess) e = upload(ny, h.NY.data(), h.NY.size() * 4);
      if (e == hipSuccess) e = upload(cs, h.CS.data(), h.CS.size() * 4);
      if (e != hipSuccess) return fail(GM_EHIP, "halo tables: %s", hipGetErrorString(e));
      s->ht = HaloTabs{pb, ny, cs, s->hg.NG, s->hg.NYn, s->hg.top};
      s->halo_send = (uint32_t*)(base + halo_tab_bytes(s->hg));
      s->halo_recv = s->halo_send + s->hg.nb * 2 * s->hg.Z;
    }
    off += h.hbytes + (s->colperm ? col_bytes(d) : 0);
    const GroupGeom gg = group_geom(d, s->world);
    const size_t gbytes = gg.on ? (group_entries(d, gg) * 4 + 255) / 256 * 256 : 0;
    if (gg.on && !s->view.blk && buf->scratch_bytes >= off + gbytes) {
      const std::vector<uint32_t> list = dense_group_lists(s, gg, gbytes / 4);
      uint32_t* dl = (uint32_t*)((char*)buf->scratch + off);
      e = list.empty() ? hipSuccess : upload(dl, list.data(), list.size() * 4);
      if (e != hipSuccess) return fail(GM_EHIP, "group lists: %s", hipGetErrorString(e));
      s->glist = dl;
    }
  }
  return dense_choose(s);
}

// Blocks of 256 threads of `kernel` that fit on the device at once (a
// multiple of 8, one share per XCD): list sweeps launch exactly that many,
// since blocks that start late would sweep their grid-stride items out of
// order.  Cached per kernel.
static int resident_blocks(const void* kernel) {
  static std::mutex mu;
  static std::map<const void*, int> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(kernel);
  if (it != cache.end()) return it->second;
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0) != hipSuccess || per_cu < 1) per_cu = 2;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  const int r = std::max(8, (per_cu * cus) & ~7);
  cache[kernel] = r;
  return r;
}

// Column jobs of level L over a shard view's listed slices: each slice's
// live columns are one range of the digit-sum-sorted permutation.  False
// if no column is live.
static bool build_col_jobs(const gm_solver* s, const DenseView& v, u64 L, ColJobs& J) {
  J.n = 0;
  J.cum[0] = 0;
  const int64_t S = (int64_t)s->d.root_sum - (int64_t)L;
  for (uint32_t i = 0; i < v.nsl; i++) {
    const int64_t t = (int64_t)v.st[i];
    const int64_t hi = std::min<int64_t>(S - t, s->cg.maxgs);
    const int64_t lo = std::max<int64_t>(S - t - (int64_t)s->d.heap[0] - s->cg.mj, 0);
    if (hi < lo) continue;
    const uint32_t a = s->cstart[(size_t)lo], b = s->cstart[(size_t)hi + 1];
    if (a == b) continue;
    J.lo[J.n] = a;
    J.u[J.n] = (uint32_t)v.sl[i];
    J.t[J.n] = (uint32_t)t;
    J.cum[J.n + 1] = J.cum[J.n] + (b - a);
    J.n++;
  }
  return J.n > 0;
}

// Forward (pull): power-of-two tables run one thread per 64-prefix bitmap
// word (k_dense_pull_words; world 1 over the level's live-group list), other
// bases one prefix per lane (k_dense_pull).
template <int MAXH, bool POW2>
static void dense_launch_pull_t(gm_solver* s, const DenseView& v, int grid, u64 L, u64 root_p) {
  if (POW2 && s->pk == PK_WORDS) {
    const uint32_t* gl = nullptr;
    u64 groups = (v.p_hi - v.p_lo + 63) / 64;
    XcdShares xs{};
    int g;
    if (s->glist && !v.blk) {  // the level's live 256-prefix groups, one share per XCD
      gl = s->glist + s->goff[L];
      if (s->goff[L + 1] == s->goff[L]) return;
      uint32_t widest = 0;
      for (int x = 0; x < 9; x++) xs.o[x] = s->gxcd[(size_t)L * 9 + x];
      for (int x = 0; x < 8; x++) widest = std::max(widest, xs.o[x + 1] - xs.o[x]);
      const u64 per = ((u64)widest * 4 + kBlock - 1) / kBlock;  // blocks per XCD
      g = (int)(kXcds * std::min<u64>(per, (u64)s->grid / kXcds));
    } else {
      g = (int)std::min<u64>((groups + kBlock - 1) / kBlock, (u64)s->grid);
    }
    hipLaunchKernelGGL((k_dense_pull_words<MAXH>), dim3(g), dim3(kBlock), 0, s->stream, s->d, v, s->bits, L,
                       root_p, s->masks, gl, xs);
    return;
  }
  hipLaunchKernelGGL((k_dense_pull<MAXH, POW2>), dim3(grid), dim3(kBlock), 0, s->stream, s->d, v, s->bits, L,
                     root_p);
}
// Backward (resolve) by the family fixed at creation (s->rk, dense_choose).
template <int MAXH, bool POW2>
static void dense_launch_resolve_t(gm_solver* s, const DenseView& v, int grid, u64 L) {
  if constexpr (POW2 && MAXH >= 2) {
    if (s->rk != RK_SCALAR) {
      const uint32_t* gl = nullptr;
      u64 units = (v.p_hi - (v.p_lo & ~255ull) + 3) / 4;
      if (s->glist && !v.blk) {  // live groups of level L, 64 units each
        gl = s->glist + s->goff[L];
        units = (s->goff[L + 1] - s->goff[L]) * 64;
        if (!units) return;
      }
      const int resident = resident_blocks((const void*)k_dense_resolve4<MAXH, false>);
      // shards: column jobs over the level's listed slices (a view that
      // lists no slices -- too many to list -- takes the band sweep)
      if constexpr (MAXH >= 3) {
        if (v.blk && s->colperm && v.nsl > 0 && v.nsl <= (uint32_t)kMaxColJobs) {
          ColJobs J;
          if (!build_col_jobs(s, v, L, J)) return;
          const RowGeom rg{v.Wl, v.Wbl, v.Z};
          if (s->w16) {  // 16-bit shard table: octets, two columns per wave
            const u64 cu8 = (u64)((J.cum[J.n] + 1) / 2) * 64;
            const int g8 = (int)std::min<u64>(
                std::min<u64>(((cu8 + kBlock - 1) / kBlock + 7) & ~7ull,
                              (u64)resident_blocks((const void*)k_dense_resolve8c<MAXH>)),
                (u64)kCountSlots);
            hipLaunchKernelGGL((k_dense_resolve8c<MAXH>), dim3(g8), dim3(kBlock), 0, s->stream, s->d, rg,
                               (uint16_t*)s->words, s->bits, L, s->st, s->colperm, J, s->bcount);
            return;
          }
          const u64 cu = (u64)J.cum[J.n] * 64;
          const int gc = (int)std::min<u64>(((cu + kBlock - 1) / kBlock + 7) & ~7ull,
                                            (u64)resident_blocks((const void*)k_dense_resolve4c<MAXH>));
          hipLaunchKernelGGL((k_dense_resolve4c<MAXH>), dim3(gc), dim3(kBlock), 0, s->stream, s->d, rg, s->words,
                             s->bits, L, s->st, s->colperm, J);
          return;
        }
      }
      if (s->w8) {  // 8-bit table: sixteen prefixes per lane over the live-group list (world 1)
        if (!gl) {
          s->launch_err = true;
          return;
        }
        XcdShares xs;
        for (int x = 0; x < 9; x++) xs.o[x] = s->gxcd[(size_t)L * 9 + x];
        for (int x = 1; x < 8; x++) xs.o[x] &= ~3u;  // shares start at entries divisible by 4: a wave = four groups
        const u64 u16 = (u64)xs.o[8] * 16;
        const int rp = resident_blocks((const void*)k_dense_resolve16p<MAXH>);
        const int gp = (int)std::min<u64>(std::min<u64>(((u16 + kBlock - 1) / kBlock + 7) & ~7ull, (u64)rp),
                                          (u64)kCountSlots);
        hipLaunchKernelGGL((k_dense_resolve16p<MAXH>), dim3(gp), dim3(kBlock), 0, s->stream, s->d, v,
                           (uint8_t*)s->words, s->bits, L, s->st, gl, xs, s->bcount);
        return;
      }
      if (s->w16) {
        // 16-bit table: octets over the live-group list (world 1).  A 16-bit
        // shard table always lists its slices (dense_choose), so reaching
        // here without a list is a bug: flag it instead of running a kernel
        // of the wrong word width.
        if (!gl) {
          s->launch_err = true;
          return;
        }
        XcdShares xs;
        for (int x = 0; x < 9; x++) xs.o[x] = s->gxcd[(size_t)L * 9 + x];
        for (int x = 1; x < 8; x++) xs.o[x] &= ~1u;  // shares start at even entries: a wave = two whole groups
        const u64 u8 = (u64)xs.o[8] * 32;
        const int rp = resident_blocks((const void*)k_dense_resolve8p<MAXH>);
        const int gp = (int)std::min<u64>(std::min<u64>(((u8 + kBlock - 1) / kBlock + 7) & ~7ull, (u64)rp),
                                          (u64)kCountSlots);
        hipLaunchKernelGGL((k_dense_resolve8p<MAXH>), dim3(gp), dim3(kBlock), 0, s->stream, s->d, v,
                           (uint16_t*)s->words, s->bits, L, s->st, gl, xs, s->bcount);
        return;
      }
      const int g = (int)std::min<u64>(((units + kBlock - 1) / kBlock + 7) & ~7ull, (u64)resident);
      if (gl) {  // 32-bit words over the list, software-pipelined
        XcdShares xs;
        for (int x = 0; x < 9; x++) xs.o[x] = s->gxcd[(size_t)L * 9 + x];
        const int rp = resident_blocks((const void*)k_dense_resolve4p<MAXH>);
        const int gp = (int)std::min<u64>(((units + kBlock - 1) / kBlock + 7) & ~7ull, (u64)rp);
        hipLaunchKernelGGL((k_dense_resolve4p<MAXH>), dim3(gp), dim3(kBlock), 0, s->stream, s->d, v, s->words,
                           s->bits, L, s->st, gl, xs);
      } else if (v.blk)
        hipLaunchKernelGGL((k_dense_resolve4<MAXH, true>), dim3(g), dim3(kBlock), 0, s->stream, s->d, v, s->words,
                           s->bits, L, s->st, nullptr, XcdShares{});
      else
        hipLaunchKernelGGL((k_dense_resolve4<MAXH, false>), dim3(g), dim3(kBlock), 0, s->stream, s->d, v, s->words,
                           s->bits, L, s->st, nullptr, XcdShares{});
      return;
    }
  }
  if (s->w16 || s->w8) {  // never chosen with the one-prefix kernel (dense_choose)
    s->launch_err = true;
    return;
  }
  if (v.blk)
    hipLaunchKernelGGL((k_dense_resolve<MAXH, POW2, true, 1, true>), dim3(grid), dim3(kBlock), 0, s->stream, s->d,
                       v, s->words, s->bits, L, s->st);
  else if (v.Wl * 4 <= 0xFFFFFFF0ull)
    hipLaunchKernelGGL((k_dense_resolve<MAXH, POW2, true, 1, false>), dim3(grid), dim3(kBlock), 0, s->stream, s->d,
                       v, s->words, s->bits, L, s->st);
  else
    hipLaunchKernelGGL((k_dense_resolve<MAXH, POW2, false, 1, false>), dim3(grid), dim3(kBlock), 0, s->stream, s->d,
                       v, s->words, s->bits, L, s->st);
}
// kernels are instantiated per exact heap count 1..8 (16 = generic)
template <bool POW2>
static void dense_launch_pull_p(gm_solver* s, const DenseView& v, int grid, u64 L, u64 root_p) {
  switch (s->d.nheaps) {
    case 1: dense_launch_pull_t<1, POW2>(s, v, grid, L, root_p); break;
    case 2: dense_launch_pull_t<2, POW2>(s, v, grid, L, root_p); break;
    case 3: dense_launch_pull_t<3, POW2>(s, v, grid, L, root_p); break;
    case 4: dense_launch_pull_t<4, POW2>(s, v, grid, L, root_p); break;
    case 5: dense_launch_pull_t<5, POW2>(s, v, grid, L, root_p); break;
    case 6: dense_launch_pull_t<6, POW2>(s, v, grid, L, root_p); break;
    case 7: dense_launch_pull_t<7, POW2>(s, v, grid, L, root_p); break;
    case 8: dense_launch_pull_t<8, POW2>(s, v, grid, L, root_p); break;
    default: dense_launch_pull_t<16, POW2>(s, v, grid, L, root_p); break;
  }
}
template <bool POW2>
static void dense_launch_resolve_p(gm_solver* s, const DenseView& v, int grid, u64 L) {
  switch (s->d.nheaps) {
    case 1: dense_launch_resolve_t<1, POW2>(s, v, grid, L); break;
    case 2: dense_launch_resolve_t<2, POW2>(s, v, grid, L); break;
    case 3: dense_launch_resolve_t<3, POW2>(s, v, grid, L); break;
    case 4: dense_launch_resolve_t<4, POW2>(s, v, grid, L); break;
    case 5: dense_launch_resolve_t<5, POW2>(s, v, grid, L); break;
    case 6: dense_launch_resolve_t<6, POW2>(s, v, grid, L); break;
    case 7: dense_launch_resolve_t<7, POW2>(s, v, grid, L); break;
    case 8: dense_launch_resolve_t<8, POW2>(s, v, grid, L); break;
    default: dense_launch_resolve_t<16, POW2>(s, v, grid, L); break;
  }
}
static void dense_launch_pull(gm_solver* s, const DenseView& v, int grid, u64 L, u64 root_p) {
  if (s->d.pow2) dense_launch_pull_p<true>(s, v, grid, L, root_p);
  else dense_launch_pull_p<false>(s, v, grid, L, root_p);
}
static void dense_launch_resolve(gm_solver* s, const DenseView& v, int grid, u64 L) {
  if (s->d.pow2) dense_launch_resolve_p<true>(s, v, grid, L);
  else dense_launch_resolve_p<false>(s, v, grid, L);
}

// Tail runs (world 1, lists; gm_dense.h k_dense_pull_tail /
// k_dense_resolve16_tail): one workgroup walks the run's levels
template <int MAXH>
static void dense_launch_tail_t(gm_solver* s, const TailRun& R, bool pull, u64 root_p) {
  if (pull) {
    hipLaunchKernelGGL((k_dense_pull_tail<MAXH>), dim3(1), dim3(kTailThreads), 0, s->stream, s->d, s->view, s->bits,
                       root_p, s->masks, s->glist, R);
    return;
  }
  if constexpr (MAXH >= 2)
    hipLaunchKernelGGL((k_dense_resolve16_tail<MAXH>), dim3(1), dim3(kTailThreads), 0, s->stream, s->d, s->view,
                       (uint8_t*)s->words, s->bits, s->st, s->glist, R, s->bcount);
  else
    s->launch_err = true;
}
static void dense_launch_tail(gm_solver* s, const TailRun& R, bool pull, u64 root_p) {
  if (!R.n) return;
  switch (s->d.nheaps) {
    case 1: dense_launch_tail_t<1>(s, R, pull, root_p); break;
    case 2: dense_launch_tail_t<2>(s, R, pull, root_p); break;
    case 3: dense_launch_tail_t<3>(s, R, pull, root_p); break;
    case 4: dense_launch_tail_t<4>(s, R, pull, root_p); break;
    case 5: dense_launch_tail_t<5>(s, R, pull, root_p); break;
    case 6: dense_launch_tail_t<6>(s, R, pull, root_p); break;
    case 7: dense_launch_tail_t<7>(s, R, pull, root_p); break;
    case 8: dense_launch_tail_t<8>(s, R, pull, root_p); break;
    default: dense_launch_tail_t<16>(s, R, pull, root_p); break;
  }
}

// Band of level L: every non-hole slot has digit sum s(p) in [S - H0, S]
// (S = root_sum - L), so its prefix lies between the smallest prefix with
// s >= S - H0 (fill the low digits first) and the largest with s <= S (fill
// the high digits first).  Narrowing a launch to the band skips whole
// stretches of holes at both ends of the tier sequence.  Returns the view
// clipped to the band (64-aligned start) or one with p_lo == p_hi.
static DenseView dense_band(const Desc& d, const DenseView& v, u64 L) {
  const int64_t S = (int64_t)d.root_sum - (int64_t)L;
  int64_t T = S - (int64_t)d.heap[0];
  u64 pmin = 0, pmax = 0;
  int64_t rem = S;
  for (int i = d.nheaps - 1; i >= 1; i--) {
    const int64_t h = std::min<int64_t>(rem, d.heap[i]);
    pmax += (u64)h * d.pstride[i];
    rem -= h;
  }
  for (int i = 1; i < d.nheaps && T > 0; i++) {
    const int64_t h = std::min<int64_t>(T, d.heap[i]);
    pmin += (u64)h * d.pstride[i];
    T -= h;
  }
  DenseView b = v;
  if (S < 0 || T > 0) {  // no slot of this level exists
    b.p_hi = b.p_lo;
    return b;
  }
  b.p_lo = std::max<u64>(v.p_lo, pmin & ~63ull);
  b.p_hi = std::min<u64>(v.p_hi, pmax + 1);
  if (b.p_hi < b.p_lo) b.p_hi = b.p_lo;
  return b;
}

// Halo exchanges of a dense shard group (block layout, DenseView).  Block
// k's bottom two own slices (top values kB, kB+1) are the upper halo of
// block k-1 (reach bits, after the pull); its top two own slices are the
// lower halo of block k+1 (words, after the resolve).  With blocks dealt
// round robin every block of rank r sends to the same neighbour rank
// (r -/+ 1 mod world), in block order, and the receiver walks its blocks in
// the same order.  Only the part of a slice pair inside level L's band
// travels: bits as whole 64-bit words, words packed to their non-hole slots
// (power-of-two tables, k_halo_move) or as the band's 4-B run.  `cs` is the
// stream the exchange runs on; each exchange lists its ranges once and hands
// them to the transport of the solve's mode (gm_xchg.h).

// prefixes [lo, hi) (offsets inside the slice pair starting at top value
// t0) of level L's band; false if none
static bool band_pair(const gm_solver* s, u64 L, int64_t t0, u64* lo, u64* hi) {
  const DenseView all{0, ~0ull, 0, 0, 0};
  const DenseView band = dense_band(s->d, all, L);
  const int64_t Z = (int64_t)s->view.Z;
  const int64_t a = std::max<int64_t>(t0 * Z, (int64_t)band.p_lo);
  const int64_t b = std::min<int64_t>((t0 + 2) * Z, (int64_t)std::min<u64>(band.p_hi, (u64)INT64_MAX));
  if (b <= a) return false;
  *lo = (u64)(a - t0 * Z);
  *hi = (u64)(b - t0 * Z);
  return true;
}

// shard s's neighbour ranks
static int ring_down(const gm_solver* s) { return (s->rank + s->world - 1) % s->world; }
static int ring_up(const gm_solver* s) { return (s->rank + 1) % s->world; }
// one halo exchange, up or down the ring, of the ranges x (x[g]: shard
// ss[g]'s lists): a group's device copies, or this process's one shard over
// its transport -- the host transport in ONE paired transfer
static int exchange_ranges(std::vector<gm_solver*>& ss, Xchg mode, hipStream_t cs, const std::vector<XLists>& x, bool up,
                           const char* what) {
  if (xchg_group(mode)) return xchg_copies(ss, mode, cs, x);
  gm_solver* s = ss[0];
  const XRound ring = up ? XRound{ring_up(s), ring_down(s)} : XRound{ring_down(s), ring_up(s)};
  return xchg_ranges(s, mode, cs, x[0], {ring}, what);
}

// after pull(L): bits of every block's bottom two own slices go down (to
// block k-1, the upper halo there)
static int exchange_bits(std::vector<gm_solver*>& ss, u64 L, Xchg mode, hipStream_t cs) {
  auto bits_at = [&](gm_solver* s, u64 j, u64 o, u64 off) {
    return s->bits + (L * s->view.Wbl + blk_slice(s, j, o) * s->view.Z + off) / 64;
  };
  std::vector<XLists> x(ss.size());
  for (size_t g = 0; g < ss.size(); g++) {
    gm_solver* s = ss[g];
    const u64 nb = blk_count(s), B = s->view.B;
    for (u64 j = 0; j < nb; j++) {
      u64 lo, hi;
      if (blk_global(s, j) >= 1 && band_pair(s, L, blk_top(s, j, 2), &lo, &hi)) {
        lo &= ~63ull;
        hi = (hi + 63) & ~63ull;
        x[g].out.push_back({ring_down(s), bits_at(s, j, 2, lo), (hi - lo) / 8});
      }
      if (blk_global(s, j) + 1 < s->nblocks && band_pair(s, L, blk_top(s, j, B + 2), &lo, &hi)) {
        lo &= ~63ull;
        hi = (hi + 63) & ~63ull;
        x[g].in.push_back({ring_up(s), bits_at(s, j, B + 2, lo), (hi - lo) / 8});
      }
    }
  }
  return exchange_ranges(ss, mode, cs, x, false, "bits halo");
}

// packed halo helpers: non-hole words of the slice pair whose first slice
// has top value t0 at level L
static uint32_t halo_total(const gm_solver* s, int64_t x) {
  return (x < 0 || x >= s->hg.XN) ? 0u : s->halo_tot[(size_t)x];
}
static uint32_t halo_count(const gm_solver* s, u64 L, int64_t t0) {
  const int64_t x0 = (int64_t)s->d.root_sum - (int64_t)L - t0;
  return halo_total(s, x0) + halo_total(s, x0 - 1);
}
// Pack (send side: every block's top pair, o = B) or unpack (receive side:
// every block's lower halo, o = 0) all of a rank's halo pairs of level L
// between the table and buf; returns the words moved.  Blocks without a
// neighbour on that side are skipped, in the same order on both ends.
static u64 halo_move_all(gm_solver* s, u64 L, int pack, uint32_t* buf, hipStream_t cs) {
  const u64 nb = blk_count(s), B = s->view.B;
  const int64_t S = (int64_t)s->d.root_sum - (int64_t)L;
  const int H0 = (int)s->d.heap[0];
  HaloColJobs J;
  J.n = 0;
  J.cum[0] = 0;
  u64 at = 0;
  auto flush = [&]() {
    if (!J.n) return;
    const u64 units = (u64)J.cum[J.n] * 64;
    const int grid = (int)std::min<u64>(((units + kBlock - 1) / kBlock + 7) & ~7ull, (u64)s->grid);
    uint32_t* lw = s->words + L * s->view.Wl;
    uint16_t* lw16 = (uint16_t*)s->words + L * s->view.Wl;
    if (s->w16) {  // two columns per wave, eight slots per lane
      const u64 u2 = (u64)((J.cum[J.n] + 1) / 2) * 64;
      const int g2 = (int)std::min<u64>(((u2 + kBlock - 1) / kBlock + 7) & ~7ull, (u64)s->grid);
      if (pack)
        hipLaunchKernelGGL((k_halo_cols16<true>), dim3(g2), dim3(kBlock), 0, cs, s->d, J, s->view.Z, s->colperm,
                           s->ht, lw16, (uint16_t*)buf);
      else
        hipLaunchKernelGGL((k_halo_cols16<false>), dim3(g2), dim3(kBlock), 0, cs, s->d, J, s->view.Z, s->colperm,
                           s->ht, lw16, (uint16_t*)buf);
    } else if (pack && s->halo16)
      hipLaunchKernelGGL((k_halo_cols<true, true>), dim3(grid), dim3(kBlock), 0, cs, s->d, J, s->view.Z, s->colperm,
                         s->ht, lw, (void*)buf);
    else if (pack)
      hipLaunchKernelGGL((k_halo_cols<true, false>), dim3(grid), dim3(kBlock), 0, cs, s->d, J, s->view.Z, s->colperm,
                         s->ht, lw, (void*)buf);
    else if (s->halo16)
      hipLaunchKernelGGL((k_halo_cols<false, true>), dim3(grid), dim3(kBlock), 0, cs, s->d, J, s->view.Z, s->colperm,
                         s->ht, lw, (void*)buf);
    else
      hipLaunchKernelGGL((k_halo_cols<false, false>), dim3(grid), dim3(kBlock), 0, cs, s->d, J, s->view.Z,
                         s->colperm, s->ht, lw, (void*)buf);
    J.n = 0;
  };
  for (u64 j = 0; j < nb; j++) {
    const u64 k = blk_global(s, j);
    if (pack ? k + 1 >= s->nblocks : k < 1) continue;
    const u64 o = pack ? B : 0;
    for (u64 m = 0; m < 2; m++) {
      const int64_t t = blk_top(s, j, o + m), x = S - t;
      const uint32_t n = halo_total(s, x);
      if (!n) continue;
      // live columns of slice x: sums gs in [x - heap0 - mj, x]
      const int64_t glo = std::max<int64_t>(0, x - H0 - s->hg.mj), ghi = std::min<int64_t>(x, s->hg.NG - 2);
      const uint32_t ca = s->cstart[(size_t)glo], cb = s->cstart[(size_t)ghi + 1];
      if (J.n == (uint32_t)kMaxHaloColJobs) flush();
      J.lo[J.n] = ca;
      J.u[J.n] = (uint32_t)blk_slice(s, j, o + m);
      J.x[J.n] = (int32_t)x;
      J.base[J.n] = (uint32_t)at;
      J.cum[J.n + 1] = J.cum[J.n] + (cb - ca);
      J.n++;
      at += n;
    }
  }
  flush();
  return at;
}
static u64 halo_recv_count(const gm_solver* s, u64 L) {
  u64 n = 0;
  for (u64 j = 0; j < blk_count(s); j++)
    if (blk_global(s, j) >= 1) n += halo_count(s, L, blk_top(s, j, 0));
  return n;
}
// words halo_move_all packs on the send side (its count, without the kernels)
static u64 halo_send_count(const gm_solver* s, u64 L) {
  u64 n = 0;
  for (u64 j = 0; j < blk_count(s); j++)
    if (blk_global(s, j) + 1 < s->nblocks) n += halo_count(s, L, blk_top(s, j, s->view.B));
  return n;
}

// Fail-fast check of a sharded solve's exchange plan.  Every message of
// every level is fixed by the geometry, so before level 0 each rank
// fingerprints, per level, the ordered byte counts it will send and receive
// for the bits (down) and words (up) halos; the fingerprints are gathered
// and a sender's must equal its receiver's.  A mismatch -- which under RCCL
// would leave a receive of the wrong size waiting forever -- is GM_ECORRUPT
// on every rank at once, before any transfer.
struct SigAcc {
  u64 h = 1469598103934665603ull, n = 0;
  void add(u64 bytes) {
    h = (h ^ bytes) * 1099511628211ull;
    n++;
  }
  u64 get() const { return h ^ (n << 56); }
};
static void halo_sigs(const gm_solver* s, u64 L, u64 out[4]) {
  SigAcc bs, br, ws, wr;
  const u64 nb = blk_count(s), B = s->view.B;
  for (u64 j = 0; j < nb; j++) {
    u64 lo, hi;
    if (blk_global(s, j) >= 1 && band_pair(s, L, blk_top(s, j, 2), &lo, &hi))
      bs.add(((hi + 63) & ~63ull) / 8 - (lo & ~63ull) / 8);
    if (blk_global(s, j) + 1 < s->nblocks && band_pair(s, L, blk_top(s, j, B + 2), &lo, &hi))
      br.add(((hi + 63) & ~63ull) / 8 - (lo & ~63ull) / 8);
  }
  if (s->hg.on) {
    const u64 wb = s->halo16 ? 2 : 4;
    const u64 ns = halo_send_count(s, L), nr = halo_recv_count(s, L);
    if (ns) ws.add(ns * wb);
    if (nr) wr.add(nr * wb);
  } else {
    for (u64 j = 0; j < nb; j++) {
      u64 lo, hi;
      if (blk_global(s, j) + 1 < s->nblocks && band_pair(s, L, blk_top(s, j, B), &lo, &hi)) ws.add((hi - lo) * 4);
      if (blk_global(s, j) >= 1 && band_pair(s, L, blk_top(s, j, 0), &lo, &hi)) wr.add((hi - lo) * 4);
    }
  }
  out[0] = bs.get();
  out[1] = br.get();
  out[2] = ws.get();
  out[3] = wr.get();
}
// all ranks' fingerprints, rank-major [world][T][4]: bits go down (rank r
// sends what r - 1 receives), words go up
static int halo_sigs_match(const std::vector<u64>& all, int world, int T) {
  auto at = [&](int r, int L, int k) { return all[((size_t)r * T + L) * 4 + k]; };
  for (int r = 0; r < world; r++) {
    const int down = (r + world - 1) % world, up = (r + 1) % world;
    for (int L = 0; L < T; L++) {
      if (at(r, L, 0) != at(down, L, 1))
        return fail(GM_ECORRUPT, "bits halo of level %d: rank %d would send what rank %d does not expect", L, r, down);
      if (at(r, L, 2) != at(up, L, 3))
        return fail(GM_ECORRUPT, "words halo of level %d: rank %d would send what rank %d does not expect", L, r, up);
    }
  }
  return 0;
}
// gather every rank's fingerprints and compare (once per solver: the
// geometry never changes)
static int check_halo_plan(std::vector<gm_solver*>& ss, Xchg mode, hipStream_t st) {
  gm_solver* s0 = ss[0];
  if (s0->halo_ok) return 0;
  const int T = s0->d.max_levels, W = s0->world;
  std::vector<u64> all;
  int rc = xchg_allgather(ss, mode, st, (size_t)T * 4, all, [&](gm_solver* s, u64* row) {
    for (int L = 0; L < T; L++) halo_sigs(s, (u64)L, &row[(size_t)L * 4]);
  });
  if (rc) return rc;
  rc = halo_sigs_match(all, W, T);
  if (rc) return rc;
  for (gm_solver* s : ss) s->halo_ok = true;
  return 0;
}

// after resolve(L): words of every block's top two own slices go up.
// Power-of-two tables send only the non-hole words (about a fifth of the
// two slices, averaged over the levels).
static int exchange_words(std::vector<gm_solver*>& ss, u64 L, Xchg mode, hipStream_t cs) {
  bool packed = true;
  for (gm_solver* s : ss) packed = packed && s->hg.on;
  auto words_at = [&](gm_solver* s, u64 j, u64 o, u64 off) {
    return s->words + L * s->view.Wl + blk_slice(s, j, o) * s->view.Z + off;
  };
  if (packed && xchg_group(mode)) {
    // every block of shard g sends to shard g + 1 (mod W): pack straight
    // into the receiver's buffer, then unpack there -- the RCCL path's
    // kernels and order, with the transfer left out
    const int W = (int)ss.size();
    for (int g = 0; g < W; g++) {
      gm_solver* dst = ss[(g + 1) % W];
      const u64 n = halo_move_all(ss[g], L, 1, dst->halo_recv, cs);
      // the RCCL path posts a receive of halo_recv_count words for the
      // sender's count: a mismatch would hang it, so the group checks it
      if (n != halo_recv_count(dst, L))
        return fail(GM_ECORRUPT, "halo count mismatch at level %llu: shard %d packs %llu, shard %d expects %llu",
                    (unsigned long long)L, g, (unsigned long long)n, (g + 1) % W,
                    (unsigned long long)halo_recv_count(dst, L));
      if (n) halo_move_all(dst, L, 0, dst->halo_recv, cs);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }
  std::vector<XLists> x(ss.size());
  if (packed) {  // one shard: its packed send buffer up, the packed receive buffer from below
    gm_solver* s = ss[0];
    if (mode == XCHG_RCCL) RCCL_LIVE(s);
    const u64 wb = s->halo16 ? 2 : 4;  // bytes per packed word
    const u64 nsend = halo_move_all(s, L, 1, s->halo_send, cs);
    HIPCHK(hipGetLastError());
    const u64 nrecv = halo_recv_count(s, L);
    x[0].out.push_back({ring_up(s), s->halo_send, nsend * wb});
    x[0].in.push_back({ring_down(s), s->halo_recv, nrecv * wb});
    int rc = exchange_ranges(ss, mode, cs, x, true, "words halo");
    if (rc) return rc;
    if (nrecv) halo_move_all(s, L, 0, s->halo_recv, cs);
    HIPCHK(hipGetLastError());
    return 0;
  }
  for (size_t g = 0; g < ss.size(); g++) {
    gm_solver* s = ss[g];
    const u64 nb = blk_count(s), B = s->view.B;
    for (u64 j = 0; j < nb; j++) {
      u64 lo, hi;
      if (blk_global(s, j) + 1 < s->nblocks && band_pair(s, L, blk_top(s, j, B), &lo, &hi))
        x[g].out.push_back({ring_up(s), words_at(s, j, B, lo), (hi - lo) * 4});
      if (blk_global(s, j) >= 1 && band_pair(s, L, blk_top(s, j, 0), &lo, &hi))
        x[g].in.push_back({ring_down(s), words_at(s, j, 0, lo), (hi - lo) * 4});
    }
  }
  int rc = exchange_ranges(ss, mode, cs, x, true, "words halo");
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// the solve: one table (world 1), one shard of an RCCL job, or every shard
// of an in-process group (all on one stream), level-synchronously
// ---------------------------------------------------------------------------
// One solve: what dense_solve_begin decides, read by the passes that run
struct DenseSolve {
  std::vector<gm_solver*>& ss;
  gm_solver* s0;
  Xchg mode = XCHG_TABLE;          // (never XCHG_STREAMS: a dense group runs on one stream)
  int T = 0, first = 0, stop = 0;  // levels; the steps [first, stop) of 2T (gm_solver_set_steps, world 1 only)
  bool timing = false;             // GM_F_KERNEL_TIMING (whole solves): ev.kx / ev.kr around shard 0's launches
  bool pipe = false;               // the halo exchanges overlap compute on the stream cs
  hipStream_t st = nullptr, cs = nullptr;
  hipEvent_t* E = nullptr;  // pipe: [0, T): own part done, [T, 2T): exchange done (forward); reused backward
  u64 root_p = 0;           // global prefix of the root (level 0)
  int slow = 0;             // largest digit sum of the prefix digits below the top
  // tail runs: per-level pulls [pa, pb), per-level resolves [rb, ra)
  int pa = 0, pb = 0, ra = 0, rb = 0;
  TailRun pull_head{}, pull_end{}, res_head{}, res_end{};
  SolveEvents ev;
  std::chrono::steady_clock::time_point t0;
  bool whole() const { return first == 0 && stop == 2 * T; }
};

// The prologue: mode and group checks, the steps, the resume check, the
// events, the pipelined exchange's stream and events, the exchange plan's
// check, the tail runs
static int dense_solve_begin(DenseSolve& c) {
  std::vector<gm_solver*>& ss = c.ss;
  gm_solver* s0 = c.s0;
  const Desc& d = s0->d;
  const int T = c.T = d.max_levels;
  int rc = xchg_mode(ss, GM_MODE_DENSE, &c.mode);
  if (rc) return rc;
  const Xchg mode = c.mode;
  if (mode == XCHG_STREAMS) return fail(GM_EINVAL, "dense group shards run on one stream");
  // forward level L is step L, backward level L is step 2T-1-L
  c.first = mode == XCHG_TABLE ? (int)s0->step_first : 0;
  c.stop = mode == XCHG_TABLE && s0->step_stop ? (int)s0->step_stop : 2 * T;
  s0->step_first = s0->step_stop = 0;
  c.timing = (s0->flags & GM_F_KERNEL_TIMING) && c.whole();
  c.st = s0->stream;
  // the kernel families and word width were fixed at creation (dense_choose);
  // a resume checks the interrupted solve used the same width
  for (gm_solver* s : ss) {
    s->launch_err = false;
    if (c.first > 0) {
      uint32_t wb = 0;
      HIPCHK(hipMemcpy(&wb, &s->st->word_bits, sizeof wb, hipMemcpyDeviceToHost));
      if (wb != 8 && wb != 16 && wb != 32) return fail(GM_EINVAL, "resume: scratch holds no solve in progress");
      if (wb != s->wbits())
        return fail(GM_EINVAL, "resume: the interrupted solve used %u-bit words, this solver %u", wb, s->wbits());
    }
  }
  if (c.ev.begin(c.timing ? (size_t)T : 0)) return GM_EHIP;
  c.root_p = d.root / d.base[0];
  c.t0 = std::chrono::steady_clock::now();
  // Sharded solves overlap each level's halo exchange with compute: a
  // level's launch is split into the part whose parents (pull) / children
  // (resolve) lie inside the shard's own block -- which includes the two
  // slices the exchange sends -- and the two boundary slices that read the
  // halo.  Per level: own part -> event -> exchange on the comm stream ->
  // event; the boundary part of the NEXT level waits for that exchange.  A
  // block narrower than 4 top values has no such split: exchange in order.
  c.pipe = mode == XCHG_RCCL || mode == XCHG_GROUP;  // the host-staged transport runs in order
  for (gm_solver* s : ss)
    if (s->view.B < 4) c.pipe = false;
  if (s0->flags & GM_F_SHARD_INORDER) c.pipe = false;  // A/B: exchange in order
  c.cs = c.st;
  if (c.pipe) {
    if (!s0->cstream) HIPCHK(hipStreamCreateWithFlags(&s0->cstream, hipStreamNonBlocking));
    while (s0->pev.size() < 2 * (size_t)T) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      s0->pev.push_back(e);
    }
    c.cs = s0->cstream;
    c.E = s0->pev.data();
  }
  for (int i = 1; i + 1 < d.nheaps; i++) c.slow += (int)d.heap[i];
  if (mode != XCHG_TABLE && (rc = check_halo_plan(ss, mode, c.st))) return rc;
  // Tail runs (one table, whole solves, live-group lists, 8-bit words): the
  // levels at both ends whose live groups fit a workgroup in a pass or two
  // run as one single-workgroup launch each (k_dense_pull_tail,
  // k_dense_resolve16_tail).  A kernel-timing solve keeps one launch per
  // level, so per-launch figures (bench roofline, PMC passes of a timed solve)
  // describe the per-level kernels alone.
  const bool tails = mode == XCHG_TABLE && !c.timing && c.whole() && s0->glist && !s0->view.blk && s0->pk == PK_WORDS &&
                     s0->w8 && d.pow2;
  c.pb = c.ra = T;
  if (tails) {
    int &pa = c.pa, &pb = c.pb, &ra = c.ra, &rb = c.rb;
    auto groups = [&](int L) { return s0->goff[(size_t)L + 1] - s0->goff[(size_t)L]; };
    auto add = [&](TailRun& R, int L) {
      R.L[R.n] = (uint32_t)L;
      R.off[R.n] = (uint32_t)s0->goff[(size_t)L];
      R.cnt[R.n] = (uint32_t)groups(L);
      R.phi[R.n] = dense_band(d, s0->view, (u64)L).p_hi;
      R.n++;
    };
    while (pa < T && pa < kTailMax && groups(pa) <= kTailPullGroups) add(c.pull_head, pa++);
    while (pb > pa && T - pb < kTailMax && groups(pb - 1) <= kTailPullGroups) pb--;
    for (int L = pb; L < T; L++) add(c.pull_end, L);
    while (ra > 0 && T - ra < kTailMax && groups(ra - 1) <= kTailResolveGroups) add(c.res_head, --ra);
    while (rb < ra && rb < kTailMax && groups(rb) <= kTailResolveGroups) rb++;
    for (int L = rb - 1; L >= 0; L--) add(c.res_end, L);
  }
  return 0;
}

// launches cover only the level's band of prefixes (dense_band); the grid is
// a multiple of 8 blocks for the XCD-chunked kernels
static int dense_grid_of(const gm_solver* s, const DenseView& b) {
  const u64 blocks = (b.p_hi - b.p_lo + kBlock - 1) / kBlock;
  return (int)std::min<u64>((blocks + 7) & ~7ull, (u64)s->grid);
}

// the launch view of level L: world 1 sweeps the level's band; a shard
// sweeps its whole local range, processing the own slices o in [olo, ohi)
// of every block
static DenseView dense_level_view(const DenseSolve& c, const gm_solver* s, int L, uint32_t olo, uint32_t ohi) {
  const Desc& d = s->d;
  if (!s->view.blk) return dense_band(d, s->view, (u64)L);
  // a shard sweeps only the listed slices of its blocks that hold a
  // non-hole at level L: top value t with 0 <= S - t <= slow + heap0
  DenseView v = s->view;
  v.olo = olo;
  v.ohi = ohi;
  const int64_t S = (int64_t)d.root_sum - L;
  uint32_t n = 0;
  bool over = false;
  for (u64 j = 0; j < blk_count(s); j++)
    for (uint32_t o = olo; o < ohi; o++) {
      const int64_t t = blk_top(s, j, o);
      if (t < 0 || (u64)t >= v.E || S - t < 0 || S - t > c.slow + (int64_t)d.heap[0]) continue;
      if (n == (uint32_t)kMaxSweepSlices || t > 0xFFFF || blk_slice(s, j, o) > 0xFFFF) {
        over = true;
      } else {
        v.sl[n] = (uint16_t)blk_slice(s, j, o);
        v.st[n++] = (uint16_t)t;
      }
    }
  v.p_lo = 0;
  if (over) {  // too many to list: sweep everything, filter per wave
    v.nsl = 0;
    v.p_hi = v.Wl;
  } else {
    v.nsl = n;
    v.p_hi = (u64)n * v.Z;
  }
  return v;
}

// forward (pull): level 0 .. T-1, each level's bitmap written exactly once.
// Parents are one or two top values ABOVE: the boundary is the top two
// slices [b-2, b), whose parents sit in the halo [b, b+2) sent down by the
// rank above.
static int dense_forward(DenseSolve& c) {
  const int T = c.T;
  const Xchg mode = c.mode;
  const bool pipe = c.pipe, timing = c.timing;
  hipStream_t st = c.st, cs = c.cs;
  hipEvent_t* E = c.E;
  if (c.first == 0) {
    for (gm_solver* s : c.ss) {
      HIPCHK(hipMemsetAsync(s->st, 0, devstate_bytes(T), st));
      HIPCHK(hipMemsetAsync(s->bcount, 0, kCountSlots * sizeof(BlockCount), st));
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&s->st->word_bits, (int)s->wbits(), 1, st));
    }
  }
  dense_launch_tail(c.s0, c.pull_head, true, c.root_p);
  for (int L = c.first; L < T && L < c.stop; L++) {
    if (L < c.pa || L >= c.pb) continue;  // in a tail run
    if (timing) HIPCHK(hipEventRecord(c.ev.kx[2 * L], st));
    for (gm_solver* s : c.ss) {
      const uint32_t B = s->view.B;  // pull: the top two own slices read the upper halo
      const DenseView own = dense_level_view(c, s, L, 2, pipe ? B : B + 2);
      if (own.p_hi > own.p_lo) dense_launch_pull(s, own, dense_grid_of(s, own), (u64)L, c.root_p);
    }
    if (mode != XCHG_TABLE) {
      if (pipe) {
        HIPCHK(hipEventRecord(E[L], st));
        HIPCHK(hipStreamWaitEvent(cs, E[L], 0));
      }
      int rc = exchange_bits(c.ss, (u64)L, mode, cs);
      if (rc) return rc;
      if (pipe) {
        HIPCHK(hipEventRecord(E[T + L], cs));
        if (L >= 1) HIPCHK(hipStreamWaitEvent(st, E[T + L - 1], 0));  // halos of L-1 (L-2 waited before)
        for (gm_solver* s : c.ss) {
          const DenseView bd = dense_level_view(c, s, L, s->view.B, s->view.B + 2);
          if (bd.p_hi > bd.p_lo) dense_launch_pull(s, bd, dense_grid_of(s, bd), (u64)L, c.root_p);
        }
      }
    }
    if (timing) HIPCHK(hipEventRecord(c.ev.kx[2 * L + 1], st));
  }
  dense_launch_tail(c.s0, c.pull_end, true, c.root_p);
  HIPCHK(hipGetLastError());
  return 0;
}

// backward (resolve): children are one or two top values BELOW: the
// boundary is the bottom two slices [a, a+2), whose children sit in the
// halo [a-2, a) sent up by the rank below.
static int dense_backward(DenseSolve& c) {
  const int T = c.T;
  const Xchg mode = c.mode;
  const bool pipe = c.pipe, timing = c.timing;
  hipStream_t st = c.st, cs = c.cs;
  hipEvent_t* E = c.E;
  dense_launch_tail(c.s0, c.res_head, false, c.root_p);
  for (int L = T - 1; L >= 0; L--) {
    if (2 * T - 1 - L < c.first) continue;
    if (2 * T - 1 - L >= c.stop) break;
    if (L >= c.ra || L < c.rb) continue;  // in a tail run
    if (timing) HIPCHK(hipEventRecord(c.ev.kr[2 * L], st));
    for (gm_solver* s : c.ss) {
      const uint32_t B = s->view.B;  // resolve: the bottom two own slices read the lower halo
      const DenseView own = dense_level_view(c, s, L, pipe ? 4 : 2, B + 2);
      if (own.p_hi > own.p_lo) dense_launch_resolve(s, own, dense_grid_of(s, own), (u64)L);
    }
    if (mode != XCHG_TABLE) {
      if (pipe) {
        HIPCHK(hipEventRecord(E[L], st));
        HIPCHK(hipStreamWaitEvent(cs, E[L], 0));
      }
      int rc = exchange_words(c.ss, (u64)L, mode, cs);
      if (rc) return rc;
      if (pipe) {
        HIPCHK(hipEventRecord(E[T + L], cs));
        if (L + 1 < T) HIPCHK(hipStreamWaitEvent(st, E[T + L + 1], 0));  // halos of L+1 (L+2 waited before)
        for (gm_solver* s : c.ss) {
          const DenseView bd = dense_level_view(c, s, L, 2, 4);
          if (bd.p_hi > bd.p_lo) dense_launch_resolve(s, bd, dense_grid_of(s, bd), (u64)L);
        }
      }
    }
    if (timing) HIPCHK(hipEventRecord(c.ev.kr[2 * L + 1], st));
  }
  dense_launch_tail(c.s0, c.res_end, false, c.root_p);
  HIPCHK(hipGetLastError());
  return 0;
}

// GM_F_GRAPH: one-table full solves replay HIP graphs of the two passes'
// launches, captured on the first such solve of the solver (every argument
// -- level views, group lists, XCD shares, tail runs, grids -- is fixed when
// the solver is made), so the host enqueues two graph launches instead of
// ~350 kernels.  Measured on the bench workload: 4.47-4.49 ms against
// 4.44-4.48 ms with plain launches (the host already runs ahead of the GPU;
// what remains between levels is the device-side kernel boundary), so it is
// not the default.  Leaves gfwd / gbwd null when a pass cannot be captured:
// a launch error is then reported by the plain path.
static int dense_graphs(DenseSolve& c) {
  gm_solver* s0 = c.s0;
  auto capture = [&](int (*issue)(DenseSolve&), hipGraphExec_t* exec) -> int {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c.st, hipStreamCaptureModeRelaxed));
    const int rc = issue(c);
    const hipError_t e = hipStreamEndCapture(c.st, &g);
    if (rc || e != hipSuccess || s0->launch_err) {
      if (g) (void)hipGraphDestroy(g);
      return rc ? rc : e != hipSuccess ? fail(GM_EHIP, "graph capture: %s", hipGetErrorString(e)) : 0;
    }
    const hipError_t ei = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
      *exec = nullptr;
      return fail(GM_EHIP, "graph instantiate: %s", hipGetErrorString(ei));
    }
    return 0;
  };
  int rc = capture(dense_forward, &s0->gfwd);
  if (!rc) rc = capture(dense_backward, &s0->gbwd);
  if (rc || !s0->gfwd || !s0->gbwd) {
    if (s0->gfwd) (void)hipGraphExecDestroy(s0->gfwd);
    if (s0->gbwd) (void)hipGraphExecDestroy(s0->gbwd);
    s0->gfwd = s0->gbwd = nullptr;
    s0->launch_err = false;
  }
  return rc;
}

// The epilogue of a whole solve: the root word and the counts of every
// shard, their reduction across the shards, the timings and the result
static int dense_finish(DenseSolve& c, gm_result* out) {
  std::vector<gm_solver*>& ss = c.ss;
  gm_solver* s0 = c.s0;
  const int T = c.T;
  const Xchg mode = c.mode;
  hipStream_t st = c.st;
  for (gm_solver* s : ss) {
    uint64_t root_q = ~0ull;
    if (!dense_local(s->view, c.root_p, &root_q)) root_q = ~0ull;
    hipLaunchKernelGGL(k_dense_root, dim3(1), dim3(64), 0, st, s->view, s->words, s->bits, root_q, s->st, s->wbits());
    hipLaunchKernelGGL(k_fill_red, dim3(1), dim3(1024), 0, st, s->st, s->bcount);
  }
  int rc = mode == XCHG_RCCL ? xchg_reduce_rccl(s0, st) : 0;
  if (rc) return rc;
  u64 red[5] = {0, 0, 0, 0, 0};  // the job's totals
  for (gm_solver* s : ss) {
    u64 r[5];
    HIPCHK(hipMemcpyAsync(r, s->st->red, sizeof r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = xchg_reduce_fold(s, mode, r, red))) return rc;
  }
  auto t1 = std::chrono::steady_clock::now();
  float f = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&f, c.ev.e0, c.ev.e1));
  HIPCHK(hipEventElapsedTime(&b, c.ev.e1, c.ev.e2));
  out->ms_forward = f;
  out->ms_backward = b;
  out->ms_total = std::chrono::duration<double, std::milli>(t1 - c.t0).count();
  if (c.timing) {
    if (SolveEvents::pairs_ms(c.ev.kx, T, &out->ms_expand_kernels)) return GM_EHIP;
    if (SolveEvents::pairs_ms(c.ev.kr, T, &out->ms_resolve_kernels)) return GM_EHIP;
    out->n_expand_launches = (uint64_t)T;
    out->n_resolve_launches = (uint64_t)T;
  }
  out->positions = red[0];
  out->edges = red[1];
  out->primitives = red[2];
  out->levels = (uint32_t)T;
  out->max_level_width = 0;
  out->word_bits = s0->wbits();
  out->kernels = s0->rk | (s0->pk << 16);
  for (gm_solver* s : ss)
    if (s->launch_err) return fail(GM_ECORRUPT, "a level found no resolve kernel of the table's word width");
  const uint32_t word = red[3] ? (uint32_t)(red[3] - 1) : NO_WORD;
  out->root_word = word;
  if (red[4]) return fail(GM_ECORRUPT, "solve failed:%s", err_text((uint32_t)red[4]).c_str());
  if (word == NO_WORD) return fail(GM_ECORRUPT, "root unresolved");
  out->root_value = (int32_t)(word & 3u);
  out->root_remoteness = word >> 2;
  return 0;
}

static int run_dense(std::vector<gm_solver*> ss, gm_result* out) {
  DenseSolve c{ss, ss[0]};
  gm_solver* s0 = c.s0;
  int rc = dense_solve_begin(c);
  if (rc) return rc;
  const bool graphed = (s0->flags & GM_F_GRAPH) && c.mode == XCHG_TABLE && !c.timing && c.whole();
  if (graphed && !s0->gfwd && (rc = dense_graphs(c))) return rc;
  const bool replay = graphed && s0->gfwd && s0->gbwd;
  hipStream_t st = c.st, cs = c.cs;
  HIPCHK(hipEventRecord(c.ev.e0, st));
  if (replay) {
    HIPCHK(hipGraphLaunch(s0->gfwd, st));
  } else if ((rc = dense_forward(c))) {
    return rc;
  }
  if (c.pipe) {  // the backward pass reuses the events: drain the forward exchanges first
    HIPCHK(hipEventRecord(c.E[0], cs));
    HIPCHK(hipStreamWaitEvent(st, c.E[0], 0));
  }
  HIPCHK(hipEventRecord(c.ev.e1, st));
  if (replay) {
    HIPCHK(hipGraphLaunch(s0->gbwd, st));
  } else if ((rc = dense_backward(c))) {
    return rc;
  }
  if (c.pipe) {  // every exchange done before the reduction and the host read-back
    HIPCHK(hipEventRecord(c.E[0], cs));
    HIPCHK(hipStreamWaitEvent(st, c.E[0], 0));
  }
  HIPCHK(hipEventRecord(c.ev.e2, st));
  if (c.stop < 2 * c.T) {  // stopped early (world 1): the state stays on the device for a resume
    HIPCHK(hipStreamSynchronize(st));
    out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c.t0).count();
    out->word_bits = s0->wbits();
    return GM_PARTIAL;
  }
  return dense_finish(c, out);
}

static int plan_dense(const Desc* d, int rank, int world, uint32_t flags, uint64_t max_table_bytes, gm_plan_t* out,
                      bool* fits) {
  DenseGeom g;
  int rc = dense_geom(d, rank, world, &g);
  if (rc) return rc;
  const u64 bytes = dense_words_bytes(d, g, dense_plan_bits(d, world, flags)) + dense_bits_bytes(d, g);
  *fits = max_table_bytes == 0 || bytes <= max_table_bytes;
  out->mode = GM_MODE_DENSE;
  out->table_slots = (u64)d->max_levels * g.v.Wl;
  out->table_bytes = bytes;
  out->level_capacity = 1;
  return 0;
}
}  // extern "C++"
