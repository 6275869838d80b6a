// gm_table.h -- the three views every reader of a table goes through, one set
// per layout, and the three readers that need nothing else
// (gm_solver_query / gm_solver_positions / gm_solver_checksum).
//
//   word of key         XxxWords   wf(d, key): the key's stored word, NO_WORD
//                                  if it has none here -- the layout's own
//                                  locate path (hashed_word, dense_word,
//                                  bk_word, plane_word<WB>, rk_word)
//   position enumerator XxxEnum    items() work items; visit(d, i, f) calls
//                                  f(key) for each position of item i
//   pair source         XxxPairs   the enumerator plus the stored words:
//                                  visit(d, i, f) calls f(key, word), the word
//                                  read where the enumeration stands -- no
//                                  lookup by key
// A layout writes its enumeration once, in XxxEnum::each(d, i, n, f): n(count)
// once per non-empty item, before its positions (the positions kernel reserves
// its output slots there), then f(key, place) per position; the place is
// whatever the layout's pair source needs to read the word.  visit() of the
// enumerator and of the pair source are adaptors over each(); what one of them
// does not use (the count, the place) is dead code in its kernels.
//
// k_query is a template over the first view, k_positions over the second,
// k_checksum over the third; gm_moves.h, gm_census.h, gm_export.h and
// gm_export_keyed.h build their kernels from the same three.
//
// Included by gm_solver.hip inside its extern "C" block, after the solver
// object and every layout header, before gm_moves.h.
extern "C++" {

// ---------------------------------------------------------------------------
// word of key, per layout
// ---------------------------------------------------------------------------
struct HashedWords {
  const gm_slot* tab;
  u64 mask;
  __device__ __forceinline__ uint32_t operator()(const Desc& d, u64 key) const { return hashed_word(d, tab, mask, key); }
};
struct DenseWords {
  DenseView v;
  const uint32_t* words;
  const u64* bits;
  uint32_t wbits;
  __device__ __forceinline__ uint32_t operator()(const Desc& d, u64 key) const {
    return dense_word(d, v, words, bits, wbits, key);
  }
};
struct BkWords {
  const u64* K;
  const uint32_t* W;
  const BkLevelDev* lv;
  int T;
  const uint32_t* meta;
  __device__ __forceinline__ uint32_t operator()(const Desc& d, u64 key) const { return bk_word(d, K, W, lv, T, meta, key); }
};
template <int WB>
struct PlaneWords {
  PlaneGeom g;
  const void* tab;
  const uint32_t* bits;
  __device__ __forceinline__ uint32_t operator()(const Desc& d, u64 key) const {
    return plane_word<WB>(d, g, tab, bits, key);
  }
};
struct RankWords {
  RankGeom g;
  __device__ __forceinline__ uint32_t operator()(const Desc&, u64 key) const { return rk_word(g, key); }
};

struct C4Words {  // RANKED, connect four (gm_ranked_connect.h)
  C4Geom g;
  __device__ __forceinline__ uint32_t operator()(const Desc&, u64 key) const { return c4_word(g, key); }
};

// ---------------------------------------------------------------------------
// position enumerators and pair sources, per layout
// ---------------------------------------------------------------------------
// kOnePerItem: item i holds exactly the i-th position (k_positions stores it
// at out[i]: the level-store order, no cursor).
struct NoCount {
  __device__ __forceinline__ void operator()(uint32_t) const {}
};
// visit() of an enumerator / of a pair source whose word of a place is word(key, place)
template <class EN, class F>
__device__ __forceinline__ void visit_keys(const EN& en, const Desc& d, u64 i, F&& f) {
  en.each(d, i, NoCount{}, [&](u64 key, auto) { f(key); });
}
template <class PS, class F>
__device__ __forceinline__ void visit_pairs(const PS& ps, const Desc& d, u64 i, F&& f) {
  ps.each(d, i, NoCount{}, [&](u64 key, auto at) { f(key, ps.word(key, at)); });
}

struct HashedEnum {  // the level key store (HASHED); place: nothing (the word is found by key)
  static constexpr bool kOnePerItem = true;
  const u64* lv;
  u64 lcap;
  const DevState* st;
  __device__ __forceinline__ u64 items() const { return st->cursor_front + st->cursor_back; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 i, N&& n, F&& f) const {
    const u64 nf = st->cursor_front;
    n(1u);
    f(i < nf ? lv[i] : lv[lcap - 1 - (i - nf)], 0);
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct HashedPairs : HashedEnum {  // the stored keys are their orbits' representatives: no any_canon
  const gm_slot* tab;
  u64 mask;
  __device__ __forceinline__ uint32_t word(u64 key, int) const {
    const u64 h = table_find(tab, mask, key);
    return h == ~0ull ? NO_WORD : tab[h].word;
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

struct FlatEnum {  // every level's keys, contiguous (BUCKETED); place: i
  static constexpr bool kOnePerItem = true;
  const u64* K;
  u64 n;
  __device__ __forceinline__ u64 items() const { return n; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 i, N&& cnt, F&& f) const {
    cnt(1u);
    f(K[i], i);
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct FlatPairs : FlatEnum {  // W[i] is the word of K[i] (bk_word reads W[L.lb + j] for K[L.lb + j])
  const uint32_t* W;
  __device__ __forceinline__ uint32_t word(u64, u64 i) const { return W[i]; }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

struct DenseEnum {  // index -> key over the whole local range, own-slice filter; place: the word's index
  static constexpr bool kOnePerItem = false;
  DenseView v;
  const u64* bits;
  u64 levels;
  __device__ __forceinline__ u64 items() const { return levels * v.Wl; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc& d, u64 i, N&& n, F&& f) const {
    const u64 L = i / v.Wl, q = i - L * v.Wl;
    bool run;
    const u64 p = dense_global(v, q, &run);
    if (!run) return;
    const int64_t h0 = dense_h0(d, L, p);
    if (h0 < 0 || !reach_bit(bits, L * v.Wbl + q)) return;
    n(1u);
    f(p * d.base[0] + (u64)h0, L * v.Wl + q);
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct DensePairs : DenseEnum {
  const uint32_t* words;
  uint32_t wbits;
  __device__ __forceinline__ uint32_t word(u64, u64 at) const { return dense_word_at(words, at, wbits); }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

struct PlaneAt {  // plane_vr's arguments
  uint32_t P, h0, h1, e;
};
template <int NO>
struct PlaneEnum {  // one plane row (32 positions) per item; the outer digit sum once per row
  static constexpr bool kOnePerItem = false;
  PlaneGeom g;
  const uint32_t* bits;
  __device__ __forceinline__ u64 items() const { return (u64)g.nplanes * 32u; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc& d, u64 i, N&& n, F&& f) const {
    const uint32_t P = (uint32_t)(i >> 5), h1 = (uint32_t)i & 31u;
    uint32_t w = plane_row_bits(bits, g, P, h1);
    if (!w) return;
    n((uint32_t)__builtin_popcount(w));
    uint32_t os;
    const u64 base = plane_key<NO>(d, g, P, 0, h1, &os);
    for (; w; w &= w - 1) {
      const uint32_t h0 = (uint32_t)__builtin_ctz(w);
      f(base + (u64)h0, PlaneAt{P, h0, h1, os + h0 + h1 + g.h1off});
    }
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
template <int NO, int WB>
struct PlanePairs : PlaneEnum<NO> {
  const void* tab;
  __device__ __forceinline__ uint32_t word(u64, const PlaneAt& a) const { return plane_vr<WB>(tab, a.P, a.h0, a.h1, a.e); }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

// (lvt: the levels' first slots [0, T], then their first block entries [T + 1, 2T + 1])
struct RankEnum {  // one 64-slot word of the reach bitmap per item; place: the slot
  static constexpr bool kOnePerItem = false;
  RankGeom g;
  const u64* lvt;
  uint32_t T;
  u64 nwords;
  __device__ __forceinline__ u64 items() const { return nwords; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 wi, N&& n, F&& f) const {
    u64 m = reinterpret_cast<const u64*>(g.reach)[wi];
    if (!m) return;
    const u64* lvstart = lvt;
    const u64* lvoff = lvt + T + 1;
    const u64 s0 = wi << 6;
    uint32_t L = 0;
    while (L + 1 < T && lvstart[L + 1] <= s0) L++;
    n((uint32_t)__builtin_popcountll(m));
    for (; m; m &= m - 1) {
      const u64 slot = s0 + (u64)__builtin_ctzll(m);
      f(rk_slot_key(g, lvstart, lvoff, L, slot), slot);
    }
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct RankPairs : RankEnum {
  __device__ __forceinline__ uint32_t word(u64, u64 slot) const { return g.words[slot]; }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

struct C4Enum {  // RANKED, connect four: one 64-slot word of the reach bitmap per item; place: the slot
  static constexpr bool kOnePerItem = false;
  C4Geom g;
  __device__ __forceinline__ u64 items() const { return g.nslots / 64; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 wi, N&& n, F&& f) const {
    u64 m = reinterpret_cast<const u64*>(g.reach)[wi];
    if (!m) return;
    const u64 s0 = wi << 6;  // (levels start 512-aligned: a word belongs to one level)
    uint32_t L = 0;
    while (L + 1 < g.T && g.lvstart[L + 1] <= s0) L++;
    n((uint32_t)__builtin_popcountll(m));
    for (; m; m &= m - 1) {
      const u64 slot = s0 + (u64)__builtin_ctzll(m);
      f(c4_slot_key(g, L, slot), slot);
    }
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct C4Pairs : C4Enum {
  __device__ __forceinline__ uint32_t word(u64, u64 slot) const { return g.words[slot]; }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

// ---------------------------------------------------------------------------
// host: the solver's layout as each of the three views
// ---------------------------------------------------------------------------
// positions of a BUCKETED table: every level's keys, contiguous in bkK / bkW
static u64 bk_positions(const gm_solver* s) {
  u64 tot = 0;
  for (const BkLevel& x : s->lvh) tot += x.n;
  return tot;
}

// f(word bytes) of an opened gmtb (1 for a gmtk, whose views read the width at run time)
template <class F>
static void tf_word_bytes_dispatch(gm_solver* s, F&& f) {
  if (s->tf_format == 2 || s->tf_wb == 1) f(std::integral_constant<int, 1>{});
  else if (s->tf_wb == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}
// f(word functor) for the solver's layout
template <class F>
static void moves_words_dispatch(gm_solver* s, F&& f) {
  if (s->mode == GM_MODE_PLANES)
    plane_form_dispatch(s, [&](auto WB, auto) {
      f(PlaneWords<decltype(WB)::value>{s->pg, (const void*)s->ptab, (const uint32_t*)s->pbits});
    });
  else if (s->mode == GM_MODE_RANKED && s->d.kind == K_CONNECT)
    f(C4Words{s->kg});
  else if (s->mode == GM_MODE_RANKED)
    f(RankWords{s->rg});
  else if (s->mode == GM_MODE_DENSE)
    f(DenseWords{s->view, s->words, s->bits, s->wbits()});
  else if (s->mode == GM_MODE_BUCKETED)
    f(BkWords{s->bkK, s->bkW, s->bkL, s->d.max_levels, s->meta});
  else if (s->mode == GM_MODE_FILE)  // an opened tablebase file (gm_table_file.h)
    tf_word_bytes_dispatch(s, [&](auto WB) {
      if (s->tf_format == 2) f(TkWords{*s->tk});
      else f(TbWords<decltype(WB)::value>{*s->tb});
    });
  else
    f(HashedWords{s->tab, s->mask});
}
// f(position enumerator) for the solver's layout
template <class F>
static void moves_enum_dispatch(gm_solver* s, F&& f) {
  if (s->mode == GM_MODE_PLANES)
    plane_no_dispatch(s->pg.no, [&](auto NO) { f(PlaneEnum<decltype(NO)::value>{s->pg, (const uint32_t*)s->pbits}); });
  else if (s->mode == GM_MODE_RANKED && s->d.kind == K_CONNECT)
    f(C4Enum{s->kg});
  else if (s->mode == GM_MODE_RANKED)
    f(RankEnum{s->rg, (const u64*)s->rlv_dev, s->rg.T, s->rg.nslots / 64});
  else if (s->mode == GM_MODE_DENSE)
    f(DenseEnum{s->view, s->bits, (u64)s->d.max_levels});
  else if (s->mode == GM_MODE_BUCKETED)
    f(FlatEnum{s->bkK, bk_positions(s)});
  else if (s->mode == GM_MODE_FILE && s->tf_format == 2)
    f(TkEnum{*s->tk});
  else if (s->mode == GM_MODE_FILE)
    f(TbEnum{*s->tb});
  else
    f(HashedEnum{s->lv, s->lcap, s->st});
}
// f(pair source) for the solver's layout: its enumerator and where the words are
template <class F>
static void pairs_of(gm_solver* s, const HashedEnum& en, F&& f) { f(HashedPairs{en, s->tab, s->mask}); }
template <class F>
static void pairs_of(gm_solver* s, const FlatEnum& en, F&& f) { f(FlatPairs{en, s->bkW}); }
template <class F>
static void pairs_of(gm_solver* s, const DenseEnum& en, F&& f) { f(DensePairs{en, s->words, s->wbits()}); }
template <int NO, class F>
static void pairs_of(gm_solver* s, const PlaneEnum<NO>& en, F&& f) {
  plane_form_dispatch(s, [&](auto WB, auto) { f(PlanePairs<NO, decltype(WB)::value>{en, (const void*)s->ptab}); });
}
template <class F>
static void pairs_of(gm_solver*, const RankEnum& en, F&& f) { f(RankPairs{en}); }
template <class F>
static void pairs_of(gm_solver*, const C4Enum& en, F&& f) { f(C4Pairs{en}); }
template <class F>
static void pairs_of(gm_solver*, const TkEnum& en, F&& f) { f(TkPairs{en}); }
template <class F>
static void pairs_of(gm_solver* s, const TbEnum& en, F&& f) {
  tf_word_bytes_dispatch(s, [&](auto WB) { f(TbPairs<decltype(WB)::value>{en}); });
}
template <class F>
static void pairs_dispatch(gm_solver* s, F&& f) {
  moves_enum_dispatch(s, [&](auto en) { pairs_of(s, en, f); });
}

// one-GPU solvers holding a finished full solve
static int moves_ready(const gm_solver* s, const char* what) {
  if (s->world > 1)
    return fail(GM_EINVAL, "%s: shard %d/%d holds part of the table (its positions' children live on other ranks); "
                           "one-GPU solvers only", what, s->rank, s->world);
  if (!s->solved) return fail(GM_EINVAL, "%s: the solver holds no finished full solve", what);
  return 0;
}

// ---------------------------------------------------------------------------
// gm_solver_query: the word of each key (NO_WORD: unreachable / not held here).
// Works on shards and on unfinished solves (the md5-sharded backward queries
// owner shards at every level), so there is no moves_ready here.
// ---------------------------------------------------------------------------
// The BUCKETED instantiation alone declares its keys and output __restrict__
// (the output aliases nothing bk_word reads): without it that kernel measured
// 2.9% slower than the k_bk_query it replaced, whose K, W, lv and meta were
// __restrict__; on every instantiation it made the RANKED query 1% slower
// (DESIGN.md 7g).  The others keep the plain pointers their old kernels had.
template <class WF>
struct QueryArgs {
  typedef const u64* keys;
  typedef uint32_t* out;
};
template <>
struct QueryArgs<BkWords> {
  typedef const u64* __restrict__ keys;
  typedef uint32_t* __restrict__ out;
};
template <class WF>
__global__ void k_query(Desc d, WF wf, typename QueryArgs<WF>::keys keys, u64 n, typename QueryArgs<WF>::out out) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
    out[i] = wf(d, keys[i]);
}

static int query_run(gm_solver* s, const uint64_t* keys_dev, uint64_t n, uint32_t* words_dev) {
  const int grid = (int)std::min<u64>((n + kBlock - 1) / kBlock, (u64)s->grid);
  moves_words_dispatch(s, [&](auto wf) {
    hipLaunchKernelGGL(k_query<decltype(wf)>, dim3(grid), dim3(kBlock), 0, s->stream, s->d, wf, (const u64*)keys_dev, n,
                       words_dev);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// gm_solver_positions: every position's key.  One cursor reservation per
// non-empty item (a PLANES row, a RANKED 64-slot word: popcount consecutive
// slots with one atomic), order arbitrary; an enumerator of one position per
// item stores item i at out[i].
// ---------------------------------------------------------------------------
template <class EN>
__global__ void k_positions(Desc d, EN en, u64* out, u64 cap, u64* count) {
  const u64 items = en.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x) {
    u64 k = i;
    en.each(
        d, i,
        [&](uint32_t c) {
          if (!EN::kOnePerItem) k = atomicAdd(count, (u64)c);
        },
        [&](u64 key, auto) {
          if (k < cap) out[k] = key;
          k++;
        });
  }
}

// *n: BUCKETED from the host's level list, HASHED both ends of the level
// store, the others the solve's position count.  keys_dev == NULL or cap < *n
// is the count query.
static int positions_run(gm_solver* s, uint64_t* keys_dev, uint64_t cap, uint64_t* n) {
  u64 cur[2] = {0, 0};
  if (s->mode == GM_MODE_BUCKETED) {
    cur[0] = bk_positions(s);
  } else if (s->mode == GM_MODE_FILE) {
    cur[0] = s->tf_format == 2 ? s->tk->positions : s->tb->positions;  // (the header's, checked at open)
  } else {
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(cur, s->st, sizeof cur, hipMemcpyDeviceToHost));  // cursor_front, cursor_back
  }
  *n = s->mode == GM_MODE_HASHED ? cur[0] + cur[1] : cur[0];
  if (*n > cap || !keys_dev) return cap < *n ? fail(GM_EFULL, "need %llu slots", (unsigned long long)*n) : 0;
  if (s->mode == GM_MODE_BUCKETED) {
    HIPCHK(hipMemcpyAsync(keys_dev, s->bkK, *n * sizeof(u64), hipMemcpyDeviceToDevice, s->stream));
  } else {
    u64* count = &s->st->cursor_back;  // (HASHED: still the level store's back end, not written)
    if (s->mode != GM_MODE_HASHED) HIPCHK(hipMemsetAsync(count, 0, sizeof(u64), s->stream));
    moves_enum_dispatch(s, [&](auto en) {
      hipLaunchKernelGGL(k_positions<decltype(en)>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, en, (u64*)keys_dev,
                         (u64)cap, count);
    });
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// gm_solver_checksum, the whole-solve fingerprint: per block partial sums of
// pos_checksum and the value histogram, one atomic per block and field
// ---------------------------------------------------------------------------
__device__ __forceinline__ void ck_block_add(u64* acc, u64 (&v)[6]) {
  __shared__ u64 part[16][6];
#pragma unroll
  for (int f = 0; f < 6; f++)
    for (int o = 32; o > 0; o >>= 1) v[f] += __shfl_xor(v[f], o);
  const int w = threadIdx.x >> 6;
  if (__lane_id() == 0)
    for (int f = 0; f < 6; f++) part[w][f] = v[f];
  __syncthreads();
  if (threadIdx.x < 6) {
    u64 t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += part[i][threadIdx.x];
    if (t) atomicAdd(&acc[threadIdx.x], t);
  }
}
__device__ __forceinline__ void ck_add(const Desc& d, u64 key, uint32_t word, u64 (&v)[6]) {
  uint8_t c[40];
  const int n = canon_from_key(d, key, c);
  v[0] += pos_checksum(c, n, word & 3u, word >> 2);
  v[1] += 1;
  // (compared, not indexed: a register-indexed v[] cost k_checksum two VGPRs over
  // the kernels it replaced, or moved the sums to LDS, by how the visitor held v)
#pragma unroll
  for (uint32_t t = 0; t < 4; t++) v[2 + t] += (word & 3u) == t;
}
template <class PS>
__global__ __launch_bounds__(256) void k_checksum(Desc d, PS ps, u64* acc) {
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  const u64 items = ps.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x)
    ps.visit(d, i, [&](u64 key, uint32_t word) { ck_add(d, key, word, v); });
  ck_block_add(acc, v);
}

static int checksum_run(gm_solver* s, uint64_t out[6]) {
  u64* acc = s->st->ck;
  HIPCHK(hipMemsetAsync(acc, 0, 6 * sizeof(u64), s->stream));
  pairs_dispatch(s, [&](auto ps) {
    hipLaunchKernelGGL(k_checksum<decltype(ps)>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, ps, acc);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, acc, 6 * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

}  // extern "C++"
