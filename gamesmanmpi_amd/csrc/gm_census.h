// gm_census.h -- the census of a solved table (gm_solver_census): positions
// by value and remoteness, by value and level, and the hardest position of
// each value.
//
// Reference path replaced: the walk a reference user does by hand over the
// resolved / remote shelves (src/cache_dict.py:44-79) to get the analysis
// table GamesmanClassic prints after a solve.
//
// Three kernels count, all into the same bins:
//   k_census<EN, WF>       any layout: the position enumerators and "word of
//                          key" functors of gm_table.h, any_level for the level
//   k_plane_census<NO, WB> PLANES in storage order: one 16-B load = 16 (8-bit
//                          words) or 8 (16-bit) positions of one row; value,
//                          remoteness and level follow from where the word is
//                          stored -- no key, no plane_locate, no division per
//                          position
//   k_rk_census            RANKED: one thread per 64-slot word of the reach
//                          bitmap, the word bytes read 16 at a time, the level
//                          from the level-start table -- no rk_slot_key
// Each has a witness form for the second pass (WIT; a runtime flag of
// k_census): it builds a key only for the positions of (value, largest
// remoteness of that value) and keeps the smallest with a 64-bit atomicMin.
//
// Bins.  A workgroup counts into u32 counters in LDS and adds them to the
// caller's u64 tables once, at its end (a workgroup sees far fewer than 2^32
// positions: the grid-stride share of a table HBM can hold).  kCensusLdsWords
// (8192 u32 = 32 KiB, five workgroups per CU) is the budget: the level table
// (4 * levels counters) goes to LDS when it fits, the remoteness table
// (4 * (rem_bins + 1)) when it fits in what is left -- so with the level
// table counted, rem_bins <= 2047 - levels stays in LDS -- and the space
// left over holds up to 4 copies of both, chosen per lane group so that lanes
// that hit the same bin in one instruction hit different copies.  In LDS a
// table is stored value-major (v * rows + row): neighbouring positions differ
// in level / remoteness by one, which then are neighbouring banks.  A table
// that does not fit is counted with 64-bit global atomics per position, that
// table only.  The largest remoteness per value is read off the finished
// remoteness table (k_census_finish); only positions in the overflow row
// carry it through an atomicMax.
//
// Included by gm_solver.hip inside its extern "C" block, after gm_moves.h.
extern "C++" {

constexpr uint32_t kCensusLdsWords = 8192;
constexpr uint32_t kCensusGlobal = 0xFFFFFFFFu;  // CensusOut::rem_off / lev_off: not in LDS
// device scratch words (gm_solver::cen_dev)
enum { CEN_COUNT = 0, CEN_MAXREM = 4, CEN_KEY = 8, CEN_BAD = 12, CEN_WORDS = 16 };

struct CensusOut {
  u64* rem;           // [(rem_bins + 1) * 4]
  u64* lev;           // [levels * 4], or null
  u64* cs;            // CEN_* words
  uint32_t rem_bins, levels;
  uint32_t rem_off, lev_off;    // first counter of the table in one LDS copy, or kCensusGlobal
  uint32_t copy_words, copies;  // counters per copy; copies: a power of two
};

// where the tables go (the header comment's rule)
static CensusOut census_layout(u64* rem, uint32_t rem_bins, u64* lev, uint32_t levels, u64* cs) {
  CensusOut o{rem, lev, cs, rem_bins, lev ? levels : 0u, kCensusGlobal, kCensusGlobal, 0, 1};
  const u64 nlev = 4ull * o.levels, nrem = 4ull * ((u64)rem_bins + 1);
  if (nlev && nlev <= kCensusLdsWords) {
    o.lev_off = 0;
    o.copy_words = (uint32_t)nlev;
  }
  if (nrem <= kCensusLdsWords - o.copy_words) {
    o.rem_off = o.copy_words;
    o.copy_words += (uint32_t)nrem;
  }
  while (o.copies < 4 && o.copy_words && 2 * o.copies * o.copy_words <= kCensusLdsWords) o.copies *= 2;
  return o;
}

__device__ __forceinline__ void census_begin(const CensusOut& o, uint32_t* hist, uint32_t* ovmx) {
  for (uint32_t i = threadIdx.x; i < o.copies * o.copy_words; i += blockDim.x) hist[i] = 0;
  if (threadIdx.x < 4) ovmx[threadIdx.x] = 0;
  __syncthreads();
}

// n positions of value v and remoteness r
__device__ __forceinline__ void census_rem(const CensusOut& o, uint32_t* hist, uint32_t copy, uint32_t v, uint32_t r,
                                           uint32_t* ovmx, uint32_t n = 1) {
  uint32_t row = r;
  if (r >= o.rem_bins) {  // the overflow row: the largest remoteness is not in the table
    row = o.rem_bins;
    atomicMax(&ovmx[v], r);
  }
  if (o.rem_off != kCensusGlobal) atomicAdd(&hist[copy * o.copy_words + o.rem_off + v * (o.rem_bins + 1) + row], n);
  else atomicAdd(&o.rem[(u64)row * 4 + v], (u64)n);
}
// n positions of value v at level L; false: L lies outside the table
__device__ __forceinline__ bool census_lev(const CensusOut& o, uint32_t* hist, uint32_t copy, uint32_t v, uint32_t L,
                                           uint32_t n = 1) {
  if (!o.levels) return true;
  if (L >= o.levels) return false;
  if (o.lev_off != kCensusGlobal) atomicAdd(&hist[copy * o.copy_words + o.lev_off + v * o.levels + L], n);
  else atomicAdd(&o.lev[(u64)L * 4 + v], (u64)n);
  return true;
}

__device__ __forceinline__ void census_end(const CensusOut& o, const uint32_t* hist, const uint32_t* ovmx, u64 bad) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < o.copy_words; i += blockDim.x) {
    u64 t = 0;
    for (uint32_t c = 0; c < o.copies; c++) t += hist[c * o.copy_words + i];
    if (!t) continue;
    if (o.rem_off != kCensusGlobal && i >= o.rem_off) {
      const uint32_t k = i - o.rem_off, v = k / (o.rem_bins + 1), row = k - v * (o.rem_bins + 1);
      atomicAdd(&o.rem[(u64)row * 4 + v], t);
    } else {
      const uint32_t v = i / o.levels, L = i - v * o.levels;
      atomicAdd(&o.lev[(u64)L * 4 + v], t);
    }
  }
  if (threadIdx.x < 4 && ovmx[threadIdx.x]) atomicMax(&o.cs[CEN_MAXREM + threadIdx.x], (u64)ovmx[threadIdx.x]);
  if (bad) atomicAdd(&o.cs[CEN_BAD], bad);
}

// the witness pass: the targets (largest remoteness per value; ~0 where the
// value has no position) and the running minimum
struct CensusTargets {
  uint32_t t[4];
  __device__ __forceinline__ void load(const u64* cs) {
    for (int v = 0; v < 4; v++) t[v] = cs[CEN_COUNT + v] ? (uint32_t)cs[CEN_MAXREM + v] : 0xFFFFFFFFu;
  }
  __device__ __forceinline__ bool match(uint32_t v, uint32_t r) const {
    return r == (v == 0 ? t[0] : v == 1 ? t[1] : v == 2 ? t[2] : t[3]);
  }
};
__device__ __forceinline__ void census_witness(u64* cs, uint32_t v, u64 key) {
  u64* w = &cs[CEN_KEY + v];
  if (key < __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(w, key);
}

__device__ __forceinline__ uint32_t u4_dword(const uint4& x, uint32_t i) {
  return i == 0 ? x.x : i == 1 ? x.y : i == 2 ? x.z : x.w;
}

// ---------------------------------------------------------------------------
// generic: enumerator + query path
// ---------------------------------------------------------------------------
// (the witness pass is a runtime flag here, not a second instantiation: one
// kernel per enumerator and functor pair, as k_audit)
template <class EN, class WF>
__global__ __launch_bounds__(256) void k_census(Desc d, EN en, WF wf, CensusOut o, bool wit) {
  __shared__ uint32_t hist[kCensusLdsWords];
  __shared__ uint32_t ovmx[4];
  CensusTargets tg;
  if (wit) tg.load(o.cs);
  else census_begin(o, hist, ovmx);
  const uint32_t copy = (threadIdx.x >> 6) & (o.copies - 1u);
  u64 bad = 0;
  const u64 items = en.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x)
    en.visit(d, i, [&](u64 key) {
      const uint32_t w = wf(d, key);
      if (w == NO_WORD) {
        bad++;
        return;
      }
      const uint32_t v = w & 3u, r = w >> 2;
      if (wit) {
        if (tg.match(v, r)) census_witness(o.cs, v, key);
      } else {
        census_rem(o, hist, copy, v, r, ovmx);
        if (!census_lev(o, hist, copy, v, (uint32_t)any_level(d, key))) bad++;
      }
    });
  if (!wit) census_end(o, hist, ovmx, bad);
}

// ---------------------------------------------------------------------------
// PLANES, in storage order
// ---------------------------------------------------------------------------
// One thread per 16-B piece: piece t of the table is plane t / PP, piece
// c = (t >> 5) % (PP / 32) of row h1 = t & 31 (gm_plane.h: plane_word_index),
// elements b = c * EPL + j of the rotated row, position h0 = (b - h1) & 31.
// A wave holds pieces of ONE plane (PP is 64 or 128): the outer digits are
// decoded once, wave-uniform.  At element step j lane l takes element
// (j + l) % EPL: the lanes of a row piece column hold digit sums e + 0 .. 15,
// so without the skew every lane of a wave would add to the same few level
// bins in one instruction; with it 16 neighbouring lanes hit 16 different
// levels, and the LDS copy is chosen by the lane's group of 16.
template <int NO, int WB, bool WIT>
__global__ __launch_bounds__(256) void k_plane_census(Desc d, PlaneGeom g, const uint4* __restrict__ tab,
                                                      const uint32_t* __restrict__ bits, CensusOut o) {
  constexpr uint32_t EPL = WB == 2 ? 8u : 16u;   // elements per load
  constexpr uint32_t PP = WB == 2 ? 128u : 64u;  // pieces per plane
  __shared__ uint32_t hist[WIT ? 1 : kCensusLdsWords];
  __shared__ uint32_t ovmx[4];
  CensusTargets tg;
  if (WIT) tg.load(o.cs);
  else census_begin(o, hist, ovmx);
  const uint32_t lane = __lane_id();
  const uint32_t copy = (lane >> 4) & (o.copies - 1u);
  u64 bad = 0;
  const u64 items = (u64)g.nplanes * PP;  // a multiple of 64: whole waves
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (u64)gridDim.x * blockDim.x) {
    const uint32_t P = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / PP));
    const uint32_t c = (uint32_t)(t >> 5) & (PP / 32u - 1u), h1 = (uint32_t)t & 31u;
    const uint32_t rowm = plane_row_bits(bits, g, P, h1);
    if (!rowm) continue;
    uint32_t dig[NO > 0 ? NO : 1], os = 0;
    plane_global_digits<NO>(g, P, dig);
#pragma unroll
    for (int j = 0; j < NO; j++) os += dig[j];
    const uint4 x = tab[t];
    u64 rowkey = 0;
    if (WIT) rowkey = plane_key<NO>(d, g, P, 0, h1);
#pragma unroll
    for (uint32_t j = 0; j < EPL; j++) {
      const uint32_t jj = (j + lane) & (EPL - 1u);
      const uint32_t h0 = (c * EPL + jj - h1) & 31u;
      if (!((rowm >> h0) & 1u)) continue;
      const uint32_t e = os + h1 + g.h1off + h0;
      uint32_t w;
      if (WB == 2) w = (u4_dword(x, jj >> 1) >> ((jj & 1u) * 16u)) & 0xFFFFu;
      else w = (u4_dword(x, jj >> 2) >> ((jj & 3u) * 8u)) & 0xFFu;
      const uint32_t vr = WB == 3 ? plane_rel_to_vr(w, e) : plane_word_to_vr(w, WB);
      const uint32_t v = vr & 3u, r = vr >> 2;
      if (WIT) {
        if (tg.match(v, r)) census_witness(o.cs, v, rowkey + h0);
      } else {
        census_rem(o, hist, copy, v, r, ovmx);
        if (!census_lev(o, hist, copy, v, d.root_sum - e)) bad++;
      }
    }
  }
  if (!WIT) census_end(o, hist, ovmx, bad);
}

// ---------------------------------------------------------------------------
// RANKED, one thread per 64-slot word of the reach bitmap
// ---------------------------------------------------------------------------
// A 64-slot word lies in one level (levels start 512-aligned), so the level
// counts of a word's slots are summed in a register (8 bits per value) and
// added once per word and value; the remoteness is binned per slot.  The 64
// word bytes are read as four 16-B loads, a quarter without a reached slot
// not at all.  (lvt: RankEnum's, gm_table.h.)
template <bool WIT>
__global__ __launch_bounds__(256) void k_rk_census(RankGeom g, const u64* __restrict__ lvt, uint32_t T, u64 nwords,
                                                   CensusOut o) {
  __shared__ uint32_t hist[WIT ? 1 : kCensusLdsWords];
  __shared__ uint32_t ovmx[4];
  CensusTargets tg;
  if (WIT) tg.load(o.cs);
  else census_begin(o, hist, ovmx);
  const u64* lvstart = lvt;
  const u64* lvoff = lvt + T + 1;
  const uint32_t copy = (threadIdx.x >> 6) & (o.copies - 1u);
  const uint4* words4 = reinterpret_cast<const uint4*>(g.words);
  u64 bad = 0;
  uint32_t L = 0;  // (wi only grows)
  for (u64 wi = (u64)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords; wi += (u64)gridDim.x * blockDim.x) {
    const u64 m = reinterpret_cast<const u64*>(g.reach)[wi];
    if (!m) continue;
    const u64 s0 = wi << 6;
    while (L + 1 < T && lvstart[L + 1] <= s0) L++;
    uint32_t pk = 0;  // slots per value, 8 bits each (a quarter adds at most 16; flushed per quarter)
    for (uint32_t q = 0; q < 4; q++) {
      uint32_t mq = (uint32_t)(m >> (16u * q)) & 0xFFFFu;
      if (!mq) continue;
      const uint4 x = words4[wi * 4 + q];
      for (; mq; mq &= mq - 1) {
        const uint32_t b = (uint32_t)__builtin_ctz(mq);
        const uint32_t w = (u4_dword(x, b >> 2) >> ((b & 3u) * 8u)) & 0xFFu;
        const uint32_t v = w & 3u, r = w >> 2;
        if (WIT) {
          if (tg.match(v, r)) census_witness(o.cs, v, rk_slot_key(g, lvstart, lvoff, L, s0 + 16u * q + b));
        } else {
          census_rem(o, hist, copy, v, r, ovmx);
          pk += 1u << (8u * v);
        }
      }
    }
    if (!WIT)
      for (uint32_t v = 0; v < 4; v++) {
        const uint32_t n = (pk >> (8u * v)) & 0xFFu;
        if (n && !census_lev(o, hist, copy, v, L, n)) bad += n;
      }
  }
  if (!WIT) census_end(o, hist, ovmx, bad);
}

// ---------------------------------------------------------------------------
// after the count: per value, the positions (the column sums of the
// remoteness table) and the largest remoteness (the last non-empty row below
// the overflow row, or what the overflow row's positions left in CEN_MAXREM);
// the witness words start at EMPTY_KEY.  One workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_census_finish(CensusOut o) {
  __shared__ u64 sum[4];
  __shared__ uint32_t mx[4];
  if (threadIdx.x < 4) {
    sum[threadIdx.x] = 0;
    mx[threadIdx.x] = 0;
  }
  __syncthreads();
  u64 a[4] = {0, 0, 0, 0};
  uint32_t top[4] = {0, 0, 0, 0};
  for (uint32_t r = threadIdx.x; r <= o.rem_bins; r += blockDim.x)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const u64 n = o.rem[(u64)r * 4 + v];
      a[v] += n;
      if (n && r < o.rem_bins) top[v] = r;  // (r only grows)
    }
#pragma unroll
  for (int v = 0; v < 4; v++) {
    if (a[v]) atomicAdd(&sum[v], a[v]);
    if (top[v]) atomicMax(&mx[v], top[v]);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int v = (int)threadIdx.x;
    o.cs[CEN_COUNT + v] = sum[v];
    o.cs[CEN_MAXREM + v] = sum[v] ? (o.cs[CEN_MAXREM + v] > mx[v] ? o.cs[CEN_MAXREM + v] : (u64)mx[v]) : 0ull;
    o.cs[CEN_KEY + v] = EMPTY_KEY;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <bool WIT>
static void census_launch(gm_solver* s, bool generic, const CensusOut& o) {
  if (!generic && s->mode == GM_MODE_PLANES) {
    const u64 items = (u64)s->pg.nplanes * (s->pform == 2 ? 128u : 64u);
    const int grid = (int)std::max<u64>(1, std::min<u64>((items + kBlock - 1) / kBlock, (u64)s->grid));
    plane_no_dispatch(s->pg.no, [&](auto NO) {
      plane_form_dispatch(s, [&](auto WB, auto) {
        hipLaunchKernelGGL((k_plane_census<decltype(NO)::value, decltype(WB)::value, WIT>), dim3(grid), dim3(kBlock), 0,
                           s->stream, s->d, s->pg, (const uint4*)s->ptab, (const uint32_t*)s->pbits, o);
      });
    });
  } else if (!generic && s->mode == GM_MODE_RANKED && s->d.kind != K_CONNECT) {
    const u64 nwords = s->rg.nslots / 64;
    const int grid = (int)std::max<u64>(1, std::min<u64>((nwords + kBlock - 1) / kBlock, (u64)s->grid));
    hipLaunchKernelGGL((k_rk_census<WIT>), dim3(grid), dim3(kBlock), 0, s->stream, s->rg, (const u64*)s->rlv_dev,
                       s->rg.T, nwords, o);
  } else {
    moves_words_dispatch(s, [&](auto wf) {
      moves_enum_dispatch(s, [&](auto en) {
        hipLaunchKernelGGL((k_census<decltype(en), decltype(wf)>), dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, en,
                           wf, o, WIT);
      });
    });
  }
}

static int census_run(gm_solver* s, uint32_t how, uint64_t* by_rem_dev, uint32_t rem_bins, uint64_t* by_level_dev,
                      uint32_t levels, uint64_t extremes[12]) {
  if (!s->cen_dev) HIPCHK(hipMalloc((void**)&s->cen_dev, CEN_WORDS * sizeof(u64)));
  const bool generic = (how & GM_CENSUS_GENERIC) != 0;
  const CensusOut o = census_layout((u64*)by_rem_dev, rem_bins, (u64*)by_level_dev, levels, s->cen_dev);
  HIPCHK(hipMemsetAsync(by_rem_dev, 0, 4 * ((size_t)rem_bins + 1) * sizeof(u64), s->stream));
  if (by_level_dev) HIPCHK(hipMemsetAsync(by_level_dev, 0, 4 * (size_t)levels * sizeof(u64), s->stream));
  HIPCHK(hipMemsetAsync(s->cen_dev, 0, CEN_WORDS * sizeof(u64), s->stream));
  census_launch<false>(s, generic, o);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_census_finish, dim3(1), dim3(256), 0, s->stream, o);
  if (extremes) census_launch<true>(s, generic, o);
  HIPCHK(hipGetLastError());
  u64 cs[CEN_WORDS];
  HIPCHK(hipMemcpyAsync(cs, s->cen_dev, sizeof cs, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (cs[CEN_BAD])
    return fail(GM_ECORRUPT, "gm_solver_census: %llu reachable position(s) without a word, or at a level outside the game's",
                (unsigned long long)cs[CEN_BAD]);
  if (extremes)
    for (int v = 0; v < 4; v++) {
      extremes[3 * v] = cs[CEN_COUNT + v];
      extremes[3 * v + 1] = cs[CEN_MAXREM + v];
      extremes[3 * v + 2] = cs[CEN_KEY + v];
    }
  return 0;
}

}  // extern "C++"
