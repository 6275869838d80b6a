// gm_export.h -- the indexed tablebase of a solved table (gm_tb_info /
// gm_tb_index / gm_solver_export): a reach bitmap over the game's index space
// plus one compact canonical word per reached index, in index order.
//
// Reference path replaced: saving a solution by walking the resolved / remote
// shelves (src/cache_dict.py:38-79), which the launcher's -sd did through
// Solver.dump(): every key to the host, every key queried back, 46 bytes per
// position before compression.
//
// A call exports indexes [first, first + count), whole 512-index blocks, in
// four steps on the solver's stream:
//   1. the reach bits of the range, one u64 per 64 indexes
//        PLANES   k_plane_export_bits: the one-bit-per-row map expanded
//        RANKED   a copy of the reach words (slot order is index order)
//        generic  k_export_generic<WF, false>: index -> key -> the layout's
//                 "word of key" functor (gm_table.h), one ballot per wave
//   2. k_export_counts: reached indexes per block (popcounts) and, per
//      workgroup of 256 blocks, their sum
//   3. k_export_scan_top / k_export_offsets: the exclusive scan over the
//      call's blocks (an LDS scan per workgroup plus one small second level)
//   4. the words, each at offset[block] + reached indexes below it in the block
//        PLANES   k_plane_export<NO, WB>: storage order, 16-B pieces as
//                 k_plane_census reads them
//        RANKED   k_rk_export: 16 word bytes per thread
//        generic  k_export_generic<WF, true>
// Step 4 is order preserving, so a workgroup's words are one contiguous run of
// the output: every kernel puts them into LDS at their place in that run
// (which also undoes the PLANES row rotation) and the workgroup stores the
// run as whole aligned 16-B pieces (export_flush); only a run's first and last
// partial piece go out bytewise.  No cursor, no atomic per position.
//
// Included by gm_solver.hip inside its extern "C" block, after gm_census.h.
extern "C++" {

// device scratch words (gm_solver::exp_dev): [EXP_WORDS | offsets[nblocks + 1] | partials]
enum { EXP_TOTAL = 0, EXP_MAXREM = 1, EXP_WORDS = 4 };
constexpr uint32_t kExportScan = 256;  // blocks per workgroup of the scan

// ---------------------------------------------------------------------------
// host: the index space
// ---------------------------------------------------------------------------
static u64 tb_sum_total(const Desc* d) { return d->stride[d->nheaps - 1] * (u64)d->base[d->nheaps - 1]; }

// the padded index space of the game; *rs (may be null): the toot shape
static int tb_space(const Desc* d, u64* space, RankShape* rs) {
  if (d->kind == K_SUM) {
    *space = (tb_sum_total(d) + GM_TB_BLOCK - 1) / GM_TB_BLOCK * GM_TB_BLOCK;
    return 0;
  }
  if (d->kind == K_TOOT && rank_ok(d)) {
    RankShape local;
    RankShape* p = rs ? rs : &local;
    const int rc = rank_shape(d, p);
    if (rc) return rc;
    *space = p->g.nslots;  // (levels padded to 512 slots)
    return 0;
  }
  return fail(GM_EINVAL, "the game has no tablebase index (rank-indexable games only: four_to_one, sum_four_to_one, "
                         "toot_and_otto_bitstring boards of the RANKED layout)");
}

// ---------------------------------------------------------------------------
// index -> key (the generic path)
// ---------------------------------------------------------------------------
struct ExportIndex {
  bool toot;
  u64 total;      // sum games: positions of the rank space (index = key)
  RankGeom g;     // toot: C, H, A, T, nslots and lvph
  const u64* lvt;  // toot: RankEnum's level tables (gm_table.h)
  __device__ __forceinline__ bool key(u64 idx, u64* out) const {
    if (!toot) {
      *out = idx;
      return idx < total;
    }
    if (idx >= g.nslots) return false;
    const u64* lvstart = lvt;
    const u64* lvoff = lvt + g.T + 1;
    uint32_t L = 0;
    while (L + 1 < g.T && lvstart[L + 1] <= idx) L++;
    const u64 i = idx - lvstart[L];
    if ((i >> (L + 3)) >= lvoff[L + 1] - lvoff[L]) return false;  // the level's padding
    const uint32_t a = (uint32_t)((i >> L) & 7u), pat = (uint32_t)(i & ((1ull << L) - 1));
    if (!rk_valid(rk_hands(L, (uint32_t)__builtin_popcount(pat), a))) return false;  // no such hands
    *out = rk_slot_key(g, lvstart, lvoff, L, idx);
    return true;
  }
};

// ---------------------------------------------------------------------------
// a workgroup's run of output words: LDS image, then aligned 16-B stores
// ---------------------------------------------------------------------------
// The image starts (o0 * wb) & 15 bytes into `lds`, so that a 16-B piece of
// the image is a 16-B aligned piece of the output (`out` is 16-B aligned).
__device__ __forceinline__ void export_put(uint8_t* lds, u64 o0, u64 pos, uint32_t w, uint32_t wb) {
  const uint32_t off = (uint32_t)((pos - o0) * wb) + ((uint32_t)(o0 * wb) & 15u);
  if (wb == 1) lds[off] = (uint8_t)w;
  else if (wb == 2) *reinterpret_cast<uint16_t*>(lds + off) = (uint16_t)w;
  else *reinterpret_cast<uint32_t*>(lds + off) = w;
}
// words [o0, o1) of the output from the image; every thread of the workgroup
__device__ __forceinline__ void export_flush(const uint8_t* lds, uint8_t* __restrict__ out, u64 o0, u64 o1,
                                             uint32_t wb) {
  __syncthreads();
  const u64 b0 = o0 * wb;
  const uint32_t sh = (uint32_t)b0 & 15u, total = (uint32_t)(o1 * wb - (b0 - sh));
  uint8_t* dst = out + (b0 - sh);
  for (uint32_t lo = threadIdx.x * 16u; lo < total; lo += blockDim.x * 16u) {
    if (lo >= sh && lo + 16u <= total) {
      *reinterpret_cast<uint4*>(dst + lo) = *reinterpret_cast<const uint4*>(lds + lo);
    } else {  // the run's first / last piece: shared with a neighbour workgroup's run
      const uint32_t a = lo > sh ? lo : sh, e = lo + 16u < total ? lo + 16u : total;
      for (uint32_t j = a; j < e; j++) dst[j] = lds[j];
    }
  }
  __syncthreads();
}
// a word that does not fit wb bytes: its remoteness to the host (rare)
__device__ __forceinline__ void export_fit(u64* xs, uint32_t w, uint32_t wb) {
  if (wb < 4 && (w >> (8u * wb))) atomicMax(&xs[EXP_MAXREM], (u64)(w >> 2));
}

// ---------------------------------------------------------------------------
// generic: one thread per index
// ---------------------------------------------------------------------------
// PUT = false: the reach bits.  PUT = true: the words (bits: step 1's, offs:
// step 3's).  count is a multiple of 512, so every wave holds one whole bits
// word and every workgroup pass half a block.
template <class WF, bool PUT>
__global__ __launch_bounds__(256) void k_export_generic(Desc d, ExportIndex ix, WF wf, u64 first, u64 count,
                                                        u64* __restrict__ bits, const u64* __restrict__ offs,
                                                        uint8_t* __restrict__ out, uint32_t wb, u64* xs) {
  __shared__ __attribute__((aligned(16))) uint8_t img[PUT ? 256 * 4 + 16 : 16];
  __shared__ u64 run[5];
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  for (u64 base = (u64)blockIdx.x * 256u; base < count; base += (u64)gridDim.x * 256u) {
    const u64 i = base + threadIdx.x;
    u64 key;
    const uint32_t w = ix.key(first + i, &key) ? wf(d, key) : NO_WORD;
    const u64 m = __ballot(w != NO_WORD);
    const u64 wi = i >> 6;
    if (!PUT) {
      if (lane == 0) bits[wi] = m;
      continue;
    }
    u64 at = offs[wi >> 3];  // the wave's first word
    for (u64 j = wi & ~7ull; j < wi; j++) at += (u64)__builtin_popcountll(bits[j]);
    if (lane == 0) {
      run[wave] = at;
      if (wave == 3) run[4] = at + (u64)__builtin_popcountll(m);
    }
    __syncthreads();
    const u64 o0 = run[0], o1 = run[4];
    if (w != NO_WORD) {
      export_fit(xs, w, wb);
      export_put(img, o0, at + (u64)__builtin_popcountll(m & ((1ull << lane) - 1ull)), w, wb);
    }
    export_flush(img, out, o0, o1, wb);
  }
}

// ---------------------------------------------------------------------------
// PLANES, in storage order
// ---------------------------------------------------------------------------
// index = key = P * 1024 + h1 * 32 + h0: a block is half a plane.  Reach is
// the one-bit-per-row map: a reached row holds h0 = 0 .. rlim[0].
__global__ __launch_bounds__(256) void k_plane_export_bits(PlaneGeom g, const uint32_t* __restrict__ rows, u64 first,
                                                           u64 nwords, u64* __restrict__ bits) {
  const u64 full = plane_row_full(g);
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (u64)gridDim.x * blockDim.x) {
    const u64 gi = (first >> 6) + i;  // rows 2k, 2k + 1 of plane gi >> 4
    const uint32_t r = rows[gi >> 4] >> (2u * ((uint32_t)gi & 15u));
    bits[i] = ((r & 1u) ? full : 0ull) | ((r & 2u) ? full << 32 : 0ull);
  }
}

// One thread per 16-B piece, as k_plane_census: piece t of the table is plane
// t / PP, piece c of row h1, elements b = c * EPL + j of the rotated row,
// position h0 = (b - h1) & 31.  A workgroup pass takes 256 / PP whole planes;
// position (h0, h1) of a reached row goes to the place of its rank in the
// output -- offset[its block] + (reached rows below it in the block's half
// plane) * (rlim[0] + 1) + h0 -- which undoes the rotation in LDS.
template <int NO, int WB>
__global__ __launch_bounds__(256) void k_plane_export(PlaneGeom g, const uint4* __restrict__ tab,
                                                      const uint32_t* __restrict__ rows, u64 first, u64 count,
                                                      const u64* __restrict__ offs, uint8_t* __restrict__ out,
                                                      uint32_t wb, u64* xs) {
  constexpr uint32_t EPL = WB == 2 ? 8u : 16u;   // elements per load
  constexpr uint32_t PP = WB == 2 ? 128u : 64u;  // pieces per plane
  constexpr uint32_t PW = 256u / PP;             // planes per workgroup pass
  __shared__ __attribute__((aligned(16))) uint8_t img[PW * 1024 * 4 + 16];
  const u64 end = first + count;
  const u64 p0 = first >> 10, p1 = (end + 1023) >> 10;
  const uint32_t per_row = g.rlim[0] >= 31 ? 32u : g.rlim[0] + 1u;
  for (u64 pw = p0 + (u64)blockIdx.x * PW; pw < p1; pw += (u64)gridDim.x * PW) {
    const u64 lo = max(first, pw << 10), hi = min(end, (pw + PW) << 10);  // this pass' indexes (workgroup-uniform)
    const u64 o0 = offs[(lo - first) >> 9], o1 = offs[(hi - first) >> 9];
    const u64 t = pw * PP + threadIdx.x;
    const uint32_t P = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / PP));
    const uint32_t c = (uint32_t)(t >> 5) & (PP / 32u - 1u), h1 = (uint32_t)t & 31u;
    const u64 row = ((u64)P << 10) + (h1 << 5);  // the row's first index: its 32 lie in one block
    const uint32_t r = P < g.nplanes && row >= first && row < end ? rows[P] : 0u;
    if ((r >> h1) & 1u) {
      uint32_t dig[NO > 0 ? NO : 1], os = 0;
      plane_global_digits<NO>(g, P, dig);
#pragma unroll
      for (int j = 0; j < NO; j++) os += dig[j];
      const uint32_t half = h1 & 16u;  // the block's rows: [half, half + 16)
      const u64 at = offs[(row - first) >> 9] +
                     (u64)__builtin_popcount((r >> half) & ((1u << (h1 & 15u)) - 1u)) * per_row;
      const uint4 x = tab[t];
#pragma unroll
      for (uint32_t j = 0; j < EPL; j++) {
        const uint32_t h0 = (c * EPL + j - h1) & 31u;
        if (h0 >= per_row) continue;
        uint32_t w;
        if (WB == 2) w = (u4_dword(x, j >> 1) >> ((j & 1u) * 16u)) & 0xFFFFu;
        else w = (u4_dword(x, j >> 2) >> ((j & 3u) * 8u)) & 0xFFu;
        const uint32_t vr = WB == 3 ? plane_rel_to_vr(w, os + h1 + g.h1off + h0) : plane_word_to_vr(w, WB);
        export_fit(xs, vr, wb);
        export_put(img, o0, at + h0, vr, wb);
      }
    }
    export_flush(img, out, o0, o1, wb);
  }
}

// ---------------------------------------------------------------------------
// RANKED: slot order is index order
// ---------------------------------------------------------------------------
// One thread per 16 slots (a quarter of a reach word, one 16-B load of word
// bytes); a workgroup pass takes 4096 slots = 8 blocks.
__global__ __launch_bounds__(256) void k_rk_export(RankGeom g, u64 first, u64 count, const u64* __restrict__ offs,
                                                   uint8_t* __restrict__ out, uint32_t wb) {
  __shared__ __attribute__((aligned(16))) uint8_t img[4096 * 4 + 16];
  __shared__ uint32_t pop[64];
  const u64* reach = reinterpret_cast<const u64*>(g.reach) + (first >> 6);
  const uint4* words4 = reinterpret_cast<const uint4*>(g.words + first);
  const u64 nblk = count >> 9;
  const uint32_t k = threadIdx.x >> 2, q = threadIdx.x & 3u;  // reach word of the pass, quarter
  for (u64 base = (u64)blockIdx.x * 4096u; base < count; base += (u64)gridDim.x * 4096u) {
    const u64 wi = (base >> 6) + k;
    const u64 m = wi < (count >> 6) ? reach[wi] : 0ull;
    if (q == 0) pop[k] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    const u64 b0 = base >> 9;
    const u64 o0 = offs[b0], o1 = offs[min(b0 + 8, nblk)];
    uint32_t mq = (uint32_t)(m >> (16u * q)) & 0xFFFFu;
    if (mq) {
      u64 at = offs[min(wi >> 3, nblk)] + (u64)__builtin_popcountll(m & ((1ull << (16u * q)) - 1ull));
      for (uint32_t j = k & ~7u; j < k; j++) at += pop[j];
      const uint4 x = words4[(base >> 4) + threadIdx.x];
      for (; mq; mq &= mq - 1, at++) {
        const uint32_t b = (uint32_t)__builtin_ctz(mq);
        export_put(img, o0, at, (u4_dword(x, b >> 2) >> ((b & 3u) * 8u)) & 0xFFu, wb);
      }
    }
    export_flush(img, out, o0, o1, wb);
  }
}

// ---------------------------------------------------------------------------
// the compaction: block counts and their exclusive scan
// ---------------------------------------------------------------------------
// inclusive scan of one value per thread over a workgroup of 256
__device__ __forceinline__ uint32_t export_wg_scan(uint32_t v, uint32_t* wsum /*[4]*/) {
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= (uint32_t)o) v += u;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  for (uint32_t j = 0; j < wave; j++) v += wsum[j];
  return v;
}
// step 2: counts[b] = reached indexes of block b; part[workgroup] = its 256 blocks' sum
__global__ __launch_bounds__(256) void k_export_counts(const u64* __restrict__ bits, u64 nblk,
                                                       uint32_t* __restrict__ counts, u64* __restrict__ part) {
  __shared__ uint32_t wsum[4];
  const u64 b = (u64)blockIdx.x * kExportScan + threadIdx.x;
  uint32_t c = 0;
  if (b < nblk) {
    const uint4* p = reinterpret_cast<const uint4*>(bits + b * 8);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint4 x = p[j];
      c += __builtin_popcount(x.x) + __builtin_popcount(x.y) + __builtin_popcount(x.z) + __builtin_popcount(x.w);
    }
    counts[b] = c;
  }
  const uint32_t inc = export_wg_scan(c, wsum);
  if (threadIdx.x == 255) part[blockIdx.x] = inc;
}
// step 3a, one workgroup: part -> its exclusive scan; the call's total
__global__ __launch_bounds__(256) void k_export_scan_top(u64* __restrict__ part, u64 nparts, u64* __restrict__ offs,
                                                         u64 nblk, u64* xs) {
  __shared__ u64 wsum[4];
  __shared__ u64 carry;
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (u64 b0 = 0; b0 < nparts; b0 += 256) {
    const u64 i = b0 + threadIdx.x;
    const u64 mine = i < nparts ? part[i] : 0ull;
    u64 v = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 u = __shfl_up(v, o);
      if (lane >= (uint32_t)o) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (uint32_t j = 0; j < wave; j++) v += wsum[j];
    const u64 c = carry;
    if (i < nparts) part[i] = c + v - mine;
    __syncthreads();
    if (threadIdx.x == 255) carry = c + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    offs[nblk] = carry;
    xs[EXP_TOTAL] = carry;
  }
}
// step 3b: offs[b] = words before block b
__global__ __launch_bounds__(256) void k_export_offsets(const uint32_t* __restrict__ counts, const u64* __restrict__ part,
                                                        u64 nblk, u64* __restrict__ offs) {
  __shared__ uint32_t wsum[4];
  const u64 b = (u64)blockIdx.x * kExportScan + threadIdx.x;
  const uint32_t c = b < nblk ? counts[b] : 0u;
  const uint32_t inc = export_wg_scan(c, wsum);
  if (b < nblk) offs[b] = part[blockIdx.x] + (inc - c);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// the RANKED index map of a toot table held in a keyed layout: the level
// tables and packed heights on the device (once per solver)
static int export_toot_geom(gm_solver* s) {
  if (s->xgeo_dev) return 0;
  RankShape rs;
  const int rc = rank_shape(&s->d, &rs);
  if (rc) return rc;
  const size_t nt = 2 * ((size_t)rs.g.T + 1), nph = rs.lvph.size();
  std::vector<u64> tabs(nt + (nph + 1) / 2, 0);
  for (uint32_t L = 0; L <= rs.g.T; L++) {
    tabs[L] = rs.lvstart[L];
    tabs[rs.g.T + 1 + L] = rs.lvoff[L];
  }
  memcpy(tabs.data() + nt, rs.lvph.data(), nph * sizeof(uint32_t));
  HIPCHK(hipMalloc((void**)&s->xgeo_dev, tabs.size() * sizeof(u64)));
  HIPCHK(hipMemcpy(s->xgeo_dev, tabs.data(), tabs.size() * sizeof(u64), hipMemcpyHostToDevice));
  s->xg = rs.g;  // (no table pointers but lvph: the index map reads nothing else)
  s->xg.lvph = reinterpret_cast<const uint32_t*>(s->xgeo_dev + nt);
  return 0;
}

static int export_run(gm_solver* s, uint32_t how, u64 first, u64 count, uint32_t wb, u64* bits, uint32_t* counts,
                      void* words, u64 cap, uint64_t* n_words) {
  const bool planes = !(how & GM_EXPORT_GENERIC) && s->mode == GM_MODE_PLANES;
  const bool ranked = !(how & GM_EXPORT_GENERIC) && s->mode == GM_MODE_RANKED;
  const u64 nblk = count / GM_TB_BLOCK, nparts = (nblk + kExportScan - 1) / kExportScan;
  const size_t need = EXP_WORDS + (size_t)nblk + 1 + (size_t)nparts;
  if (s->exp_words < need) {
    if (s->exp_dev) HIPCHK(hipFree(s->exp_dev));
    s->exp_dev = nullptr;
    s->exp_words = 0;
    HIPCHK(hipMalloc((void**)&s->exp_dev, need * sizeof(u64)));
    s->exp_words = need;
  }
  u64* xs = s->exp_dev;
  u64* offs = xs + EXP_WORDS;
  u64* part = offs + nblk + 1;
  ExportIndex ix{};
  if (!planes && !ranked) {
    ix.toot = s->d.kind == K_TOOT;
    if (!ix.toot) {
      ix.total = tb_sum_total(&s->d);
    } else if (s->mode == GM_MODE_RANKED) {
      ix.g = s->rg;
      ix.lvt = s->rlv_dev;
    } else {
      const int rc = export_toot_geom(s);
      if (rc) return rc;
      ix.g = s->xg;
      ix.lvt = s->xgeo_dev;
    }
  }
  auto grid_for = [&](u64 items) { return (int)std::max<u64>(1, std::min<u64>((items + kBlock - 1) / kBlock, (u64)s->grid)); };
  HIPCHK(hipMemsetAsync(xs, 0, EXP_WORDS * sizeof(u64), s->stream));
  // 1. the reach bits
  if (planes)
    hipLaunchKernelGGL(k_plane_export_bits, dim3(grid_for(count / 64)), dim3(kBlock), 0, s->stream, s->pg,
                       (const uint32_t*)s->pbits, first, count / 64, bits);
  else if (ranked)
    HIPCHK(hipMemcpyAsync(bits, reinterpret_cast<const u64*>(s->rg.reach) + first / 64, count / 8,
                          hipMemcpyDeviceToDevice, s->stream));
  else
    moves_words_dispatch(s, [&](auto wf) {
      hipLaunchKernelGGL((k_export_generic<decltype(wf), false>), dim3(grid_for(count)), dim3(kBlock), 0, s->stream,
                         s->d, ix, wf, first, count, bits, (const u64*)nullptr, (uint8_t*)nullptr, wb, xs);
    });
  // 2., 3. counts and offsets
  hipLaunchKernelGGL(k_export_counts, dim3((unsigned)nparts), dim3(kExportScan), 0, s->stream, (const u64*)bits, nblk,
                     counts, part);
  hipLaunchKernelGGL(k_export_scan_top, dim3(1), dim3(256), 0, s->stream, part, nparts, offs, nblk, xs);
  hipLaunchKernelGGL(k_export_offsets, dim3((unsigned)nparts), dim3(kExportScan), 0, s->stream,
                     (const uint32_t*)counts, (const u64*)part, nblk, offs);
  HIPCHK(hipGetLastError());
  u64 total = 0;
  HIPCHK(hipMemcpyAsync(&total, xs + EXP_TOTAL, sizeof total, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n_words = total;
  if (total > cap)
    return fail(GM_EFULL, "gm_solver_export: %llu words for indexes [%llu, +%llu), room for %llu",
                (unsigned long long)total, (unsigned long long)first, (unsigned long long)count, (unsigned long long)cap);
  if (!total) return 0;
  // 4. the words
  if (planes) {
    const u64 np = ((first + count + 1023) >> 10) - (first >> 10);
    plane_no_dispatch(s->pg.no, [&](auto NO) {
      plane_form_dispatch(s, [&](auto WB, auto) {
        constexpr uint32_t PW = decltype(WB)::value == 2 ? 2u : 4u;
        const int grid = (int)std::max<u64>(1, std::min<u64>((np + PW - 1) / PW, (u64)s->grid));
        hipLaunchKernelGGL((k_plane_export<decltype(NO)::value, decltype(WB)::value>), dim3(grid), dim3(kBlock), 0,
                           s->stream, s->pg, (const uint4*)s->ptab, (const uint32_t*)s->pbits, first, count,
                           (const u64*)offs, (uint8_t*)words, wb, xs);
      });
    });
  } else if (ranked) {
    const int grid = (int)std::max<u64>(1, std::min<u64>((count + 4095) / 4096, (u64)s->grid));
    hipLaunchKernelGGL(k_rk_export, dim3(grid), dim3(kBlock), 0, s->stream, s->rg, first, count, (const u64*)offs,
                       (uint8_t*)words, wb);
  } else {
    moves_words_dispatch(s, [&](auto wf) {
      hipLaunchKernelGGL((k_export_generic<decltype(wf), true>), dim3(grid_for(count)), dim3(kBlock), 0, s->stream,
                         s->d, ix, wf, first, count, bits, (const u64*)offs, (uint8_t*)words, wb, xs);
    });
  }
  HIPCHK(hipGetLastError());
  u64 maxrem = 0;
  HIPCHK(hipMemcpyAsync(&maxrem, xs + EXP_MAXREM, sizeof maxrem, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (maxrem)
    return fail(GM_EINVAL, "gm_solver_export: remoteness %llu does not fit words of %u byte(s) (value | remoteness << 2)",
                (unsigned long long)maxrem, wb);
  return 0;
}

}  // extern "C++"
