// gm_export_keyed.h -- the keyed tablebase of a solved table
// (gm_solver_export_keyed): every position's key and compact word, grouped by
// hash bucket and sorted by key inside a bucket, for the games that have no
// tablebase index (tic_tac_toe_np, mttt, othello_bit_new) and for any other
// descriptor game.
//
// Reference path replaced: saving a solution by walking the resolved / remote
// shelves (src/cache_dict.py:38-79), which the launcher's -sd did for these
// games through Solver.dump() and write_stats: every key to the host, every
// key queried back, 32 canonical bytes decoded per key, np.savez_compressed.
//
// bucket(key) = the top bucket_bits bits of mix64(key) (0 when bucket_bits is
// 0).  Four passes on the solver's stream, (key, word) pairs coming from a
// pair source -- the layout's position enumerator and "word of key" functor
// (TkLookup), or BUCKETED's own pair source, K[i] / W[i] side by side
// (FlatPairs, gm_table.h):
//   1. k_tk_count    positions per bucket (u32): a histogram in LDS, flushed
//                    once per workgroup for its non-empty bins, when the
//                    2^bucket_bits counters fit gm_census.h's LDS budget
//                    (bucket_bits <= 13); one global atomic per position
//                    otherwise.  Also the OR of all keys (-> key_bytes), the
//                    largest remoteness and the positions without a word.
//   2. k_tk_parts, k_export_scan_top, k_export_offsets (gm_export.h): the
//      exclusive scan of the counts, which IS the file's directory; k_tk_parts
//      also takes the largest bucket.
//   3. k_tk_scatter  (key, word) to staging at dir[bucket] + a per-bucket
//                    cursor (the zeroed counts): any order inside a bucket
//   4. k_tk_sort     one workgroup per bucket (grid-stride over the buckets):
//                    the bucket into LDS, padded with ~0 keys to a power of
//                    two, a bitonic sort by key carrying the word, then the
//                    truncated-key run and the word run as LDS images stored
//                    by export_flush -- aligned 16-B pieces, bytewise only at
//                    a run's two ends.  At most kTkBucketCap positions per
//                    bucket: 12 KiB of pairs + at most 12 KiB of images.
// The host checks between 2 and 3, so a refused call writes the directory
// and nothing else.
//
// Included by gm_solver.hip inside its extern "C" block, after gm_export.h.
extern "C++" {

constexpr uint32_t kTkBucketCap = 1024;  // positions of one bucket (k_tk_sort's LDS)
// device scratch (gm_solver::exp_dev): [EXP_WORDS | TK_WORDS | part[nparts] | counts u32[2^b]]
enum { TK_OR = 0, TK_BAD = 1, TK_MAXBUCKET = 2, TK_WORDS = 4 };

// (tk_bucket: gm_table_file.h, which reads the buckets back)

// ---------------------------------------------------------------------------
// the pair source (gm_table.h) that reads nothing in place: the deliberately
// independent path GM_EXPORT_GENERIC keeps
// ---------------------------------------------------------------------------
template <class EN, class WF>
struct TkLookup {  // any layout: enumerate the keys, look each word up
  EN en;
  WF wf;
  __device__ __forceinline__ u64 items() const { return en.items(); }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    en.visit(d, i, [&](u64 key) { f(key, wf(d, key)); });
  }
};

// ---------------------------------------------------------------------------
// 1. count
// ---------------------------------------------------------------------------
// lds: 2^b <= kCensusLdsWords.  counts are u32: a bucket holds far fewer than
// 2^32 positions of a table that is exported (kTkBucketCap).
template <class PS>
__global__ __launch_bounds__(256) void k_tk_count(Desc d, PS ps, uint32_t b, bool lds, uint32_t* __restrict__ counts,
                                                  u64* __restrict__ xs, u64* __restrict__ tk) {
  __shared__ uint32_t hist[kCensusLdsWords];
  const uint32_t nb = lds ? 1u << b : 0u;
  for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  u64 bad = 0, orv = 0;
  uint32_t mr = 0;
  const u64 items = ps.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x)
    ps.visit(d, i, [&](u64 key, uint32_t w) {
      if (w == NO_WORD) {
        bad++;
        return;
      }
      orv |= key;
      mr = max(mr, w >> 2);
      const u64 h = tk_bucket(key, b);
      if (lds) atomicAdd(&hist[h], 1u);
      else atomicAdd(&counts[h], 1u);
    });
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x)
    if (hist[i]) atomicAdd(&counts[i], hist[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    orv |= __shfl_xor(orv, o);
    mr = max(mr, (uint32_t)__shfl_xor(mr, o));
  }
  if (__lane_id() == 0) {
    if (orv) atomicOr(&tk[TK_OR], orv);
    if (mr) atomicMax(&xs[EXP_MAXREM], (u64)mr);
  }
  block_add(&tk[TK_BAD], bad);
}

// ---------------------------------------------------------------------------
// 2. part[workgroup] = its 256 buckets' sum (k_export_counts' second half);
// the largest bucket
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tk_parts(const uint32_t* __restrict__ counts, u64 nb, u64* __restrict__ part,
                                                  u64* __restrict__ tk) {
  __shared__ uint32_t wsum[4];
  const u64 h = (u64)blockIdx.x * kExportScan + threadIdx.x;
  const uint32_t c = h < nb ? counts[h] : 0u;
  const uint32_t inc = export_wg_scan(c, wsum);
  if (threadIdx.x == 255) part[blockIdx.x] = inc;
  uint32_t m = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor(m, o));
  if (__lane_id() == 0 && m) atomicMax(&tk[TK_MAXBUCKET], (u64)m);
}

// ---------------------------------------------------------------------------
// 3. scatter to staging: keys u64[total], then words u32[total]
// ---------------------------------------------------------------------------
template <class PS>
__global__ __launch_bounds__(256) void k_tk_scatter(Desc d, PS ps, uint32_t b, const u64* __restrict__ dir,
                                                    uint32_t* __restrict__ cur, u64* __restrict__ skeys,
                                                    uint32_t* __restrict__ swords, u64 total) {
  const u64 items = ps.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x)
    ps.visit(d, i, [&](u64 key, uint32_t w) {
      if (w == NO_WORD) return;
      const u64 h = tk_bucket(key, b);
      const u64 at = dir[h] + atomicAdd(&cur[h], 1u);
      if (at < total) {  // (the table is only read: the count pass saw the same pairs)
        skeys[at] = key;
        swords[at] = w;
      }
    });
}

// ---------------------------------------------------------------------------
// 4. sort and pack, one workgroup per bucket
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tk_sort(const u64* __restrict__ dir, u64 nb, const u64* __restrict__ skeys,
                                                 const uint32_t* __restrict__ swords, uint8_t* __restrict__ keys_out,
                                                 uint8_t* __restrict__ words_out, uint32_t kb, uint32_t wb) {
  __shared__ u64 sk[kTkBucketCap];
  __shared__ uint32_t sw[kTkBucketCap];
  __shared__ __attribute__((aligned(16))) uint8_t kimg[kTkBucketCap * 8 + 16];
  __shared__ __attribute__((aligned(16))) uint8_t wimg[kTkBucketCap * 4 + 16];
  for (u64 h = blockIdx.x; h < nb; h += gridDim.x) {
    const u64 o0 = dir[h], o1 = dir[h + 1];  // (workgroup-uniform)
    if (o1 <= o0 || o1 - o0 > kTkBucketCap) continue;
    const uint32_t n = (uint32_t)(o1 - o0);
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
      sk[i] = i < n ? skeys[o0 + i] : ~0ull;
      sw[i] = i < n ? swords[o0 + i] : 0u;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
          const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
          const u64 a = sk[i], c = sk[p];
          if ((a > c) == !(i & k)) {
            sk[i] = c;
            sk[p] = a;
            const uint32_t x = sw[i];
            sw[i] = sw[p];
            sw[p] = x;
          }
        }
        __syncthreads();
      }
    const uint32_t ksh = (uint32_t)(o0 * kb) & 15u;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const u64 key = sk[i];
      for (uint32_t j = 0; j < kb; j++) kimg[ksh + i * kb + j] = (uint8_t)(key >> (8u * j));
      export_put(wimg, o0, o0 + i, sw[i], wb);
    }
    export_flush(kimg, keys_out, o0, o1, kb);
    export_flush(wimg, words_out, o0, o1, wb);
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// f(pair source) for the solver's layout
template <class F>
static void tk_source_dispatch(gm_solver* s, bool generic, F&& f) {
  if (!generic && s->mode == GM_MODE_BUCKETED) {
    f(FlatPairs{{s->bkK, bk_positions(s)}, s->bkW});
    return;
  }
  moves_words_dispatch(s, [&](auto wf) {
    moves_enum_dispatch(s, [&](auto en) { f(TkLookup<decltype(en), decltype(wf)>{en, wf}); });
  });
}

static int export_keyed_run(gm_solver* s, uint32_t how, uint32_t b, uint32_t wb, void* stage, u64* dir, void* keys,
                            void* words, u64 cap, uint64_t out[4]) {
  const bool generic = (how & GM_EXPORT_GENERIC) != 0;
  const u64 nb = 1ull << b, nparts = (nb + kExportScan - 1) / kExportScan;
  const size_t need = EXP_WORDS + TK_WORDS + (size_t)nparts + ((size_t)nb + 1) / 2;
  if (s->exp_words < need) {
    if (s->exp_dev) HIPCHK(hipFree(s->exp_dev));
    s->exp_dev = nullptr;
    s->exp_words = 0;
    HIPCHK(hipMalloc((void**)&s->exp_dev, need * sizeof(u64)));
    s->exp_words = need;
  }
  u64* xs = s->exp_dev;
  u64* tk = xs + EXP_WORDS;
  u64* part = tk + TK_WORDS;
  uint32_t* counts = reinterpret_cast<uint32_t*>(part + nparts);
  const bool lds = nb <= kCensusLdsWords;
  HIPCHK(hipMemsetAsync(xs, 0, (EXP_WORDS + TK_WORDS) * sizeof(u64), s->stream));
  HIPCHK(hipMemsetAsync(counts, 0, nb * sizeof(uint32_t), s->stream));
  // 1. count
  tk_source_dispatch(s, generic, [&](auto ps) {
    hipLaunchKernelGGL(k_tk_count<decltype(ps)>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, ps, b, lds, counts, xs,
                       tk);
  });
  // 2. the directory
  hipLaunchKernelGGL(k_tk_parts, dim3((unsigned)nparts), dim3(kExportScan), 0, s->stream, (const uint32_t*)counts, nb,
                     part, tk);
  hipLaunchKernelGGL(k_export_scan_top, dim3(1), dim3(256), 0, s->stream, part, nparts, dir, nb, xs);
  hipLaunchKernelGGL(k_export_offsets, dim3((unsigned)nparts), dim3(kExportScan), 0, s->stream,
                     (const uint32_t*)counts, (const u64*)part, nb, dir);
  HIPCHK(hipGetLastError());
  u64 hs[EXP_WORDS + TK_WORDS];
  HIPCHK(hipMemcpyAsync(hs, xs, sizeof hs, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  const u64 total = hs[EXP_TOTAL], maxrem = hs[EXP_MAXREM], orv = hs[EXP_WORDS + TK_OR];
  const u64 bad = hs[EXP_WORDS + TK_BAD], maxbucket = hs[EXP_WORDS + TK_MAXBUCKET];
  uint32_t kb = 1;
  while (kb < 8 && (orv >> (8u * kb))) kb++;
  out[0] = total;
  out[1] = kb;
  out[2] = maxbucket;
  out[3] = maxrem;
  if (bad)
    return fail(GM_ECORRUPT, "gm_solver_export_keyed: %llu reachable position(s) without a word", (unsigned long long)bad);
  if (wb < 4 && (((maxrem << 2) | 3u) >> (8u * wb)))
    return fail(GM_EINVAL, "gm_solver_export_keyed: remoteness %llu does not fit words of %u byte(s) (value | remoteness << 2)",
                (unsigned long long)maxrem, wb);
  if (maxbucket > kTkBucketCap)
    return fail(GM_EFULL, "gm_solver_export_keyed: the largest bucket holds %llu positions at bucket_bits %u, a bucket's "
                          "capacity is %u: raise bucket_bits",
                (unsigned long long)maxbucket, b, kTkBucketCap);
  if (total > cap)
    return fail(GM_EFULL, "gm_solver_export_keyed: %llu positions, room for %llu", (unsigned long long)total,
                (unsigned long long)cap);
  if (!total) return 0;
  // 3. scatter (the counts become the cursors)
  u64* skeys = reinterpret_cast<u64*>(stage);
  uint32_t* swords = reinterpret_cast<uint32_t*>(skeys + total);
  HIPCHK(hipMemsetAsync(counts, 0, nb * sizeof(uint32_t), s->stream));
  tk_source_dispatch(s, generic, [&](auto ps) {
    hipLaunchKernelGGL(k_tk_scatter<decltype(ps)>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, ps, b,
                       (const u64*)dir, counts, skeys, swords, total);
  });
  // 4. sort and pack
  const int grid = (int)std::min<u64>(nb, (u64)s->grid);
  hipLaunchKernelGGL(k_tk_sort, dim3(grid), dim3(kBlock), 0, s->stream, (const u64*)dir, nb, (const u64*)skeys,
                     (const uint32_t*)swords, (uint8_t*)keys, (uint8_t*)words, kb, wb);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

}  // extern "C++"
