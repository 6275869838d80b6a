// gm_moves.h -- move analysis and the whole-table audit of a solved table
// (gm_solver_moves / gm_solver_line / gm_solver_audit).
//
// Reference path replaced: the walk a reference user does by hand over the
// resolved / remote shelves (src/cache_dict.py:44-79) with GameState.expand
// (src/game_state.py:58-84): expand a position, read every child's value and
// remoteness, reduce them (src/process.py _res_red / _remote_red, SURVEY §8a
// A8/A9).
//
// One device primitive serves all three calls: expand a key with the device
// descriptor (any_prim / any_children, gm_games.h), fetch every child's word
// through the layout's "word of key" functor (gm_table.h: the locate path
// gm_solver_query runs) and reduce with the reference-canonical rule
// (k_resolve).  Nothing here goes
// through the register-resident wavefronts that wrote the tables
// (k_plane_flow, k_rk_backward, k_bk_reduce, the dense resolvers), so the
// audit is an independent check of them.
//
// Included by gm_solver.hip inside its extern "C" block, after gm_table.h.
extern "C++" {

// ---------------------------------------------------------------------------
// the reduction (k_resolve's rule) and the best-move rule
// ---------------------------------------------------------------------------
// Running reduction over a position's children.  A child without a word
// (absent or unreached) makes the result NO_WORD.
struct MoveAcc {
  bool any_loss = false, any_tie = false, any_draw = false, missing = false;
  uint32_t min_loss = 0xFFFFFFFFu, max_all = 0;
  __device__ __forceinline__ void add(uint32_t w) {
    if (w == NO_WORD) {
      missing = true;
      return;
    }
    const uint32_t v = w & 3u, r = w >> 2;
    if (v == LOSS) {
      any_loss = true;
      min_loss = min(min_loss, r);
    }
    any_tie |= (v == TIE);
    any_draw |= (v == DRAW);
    max_all = max(max_all, r);
  }
  // reference-canonical _res_red / _remote_red
  __device__ __forceinline__ uint32_t word() const {
    if (missing) return NO_WORD;
    if (any_loss) return make_word(WIN, min_loss + 1);
    return make_word(any_tie ? TIE : any_draw ? DRAW : LOSS, max_all + 1);
  }
};

// Best-move score of child `i` with word `w` under a parent of value `pv`;
// the best move is the child with the SMALLEST score (ties cannot happen:
// the child's index is the low 5 bits).  ~0: not a candidate.
//   parent WIN : the first LOSS child of the smallest remoteness
//   parent TIE : the first TIE child of the largest remoteness among TIE children
//   parent DRAW: the first DRAW child
//   parent LOSS: the first child of the largest remoteness
__device__ __forceinline__ u64 move_score(int pv, uint32_t w, int i) {
  if (w == NO_WORD) return ~0ull;
  const uint32_t v = w & 3u, r = w >> 2;
  const u64 far = (u64)(0x3FFFFFFFu - r);
  switch (pv) {
    case WIN: return v == LOSS ? ((u64)r << 5) | (u64)i : ~0ull;
    case TIE: return v == TIE ? (far << 5) | (u64)i : ~0ull;
    case DRAW: return v == DRAW ? (u64)i : ~0ull;
    default: return (far << 5) | (u64)i;
  }
}

// One thread: the word the reduction gives `key` (a non-primitive position)
// from its children's stored words; *nch = its child count.
template <class WF>
__device__ __forceinline__ uint32_t reduce_children(const Desc& d, const WF& wf, u64 key, int* nch) {
  MoveAcc acc;
  *nch = any_children(d, key, [&](u64 c, int) { acc.add(wf(d, c)); });
  return *nch ? acc.word() : NO_WORD;
}

// The line walker's step (k_line: one position at a time, so the latency of
// its children's lookups is what there is to hide).  A group of 32 lanes (a
// half-wave) expands `key` (on == false: the group idles, n = 0).  Lane 0 of the group runs the descriptor's callback
// enumerator into the group's LDS row; lanes 0..n-1 then fetch their child's
// word in parallel; the reduction and the best move are cross-lane
// (__ballot over the half, __shfl_xor inside it).  Every thread of the block
// must call this together (two block barriers); self_word is the key's own
// stored word, read in the group's lane 0.  On return lane j holds
// child j / its word (EMPTY_KEY / NO_WORD for j >= n); n, best and the
// reduced word are the same in every lane of the group.  A primitive or
// unreachable key has n = 0, best = -1, reduced = NO_WORD.
struct GroupLDS {
  u64 child[MAXCHILD];
  int n;
};
template <class WF>
__device__ __forceinline__ void group_moves(const Desc& d, const WF& wf, bool on, u64 key, uint32_t self_word,
                                            GroupLDS& lds, int* n_out, u64* child_out, uint32_t* word_out,
                                            int* best_out, uint32_t* reduced_out) {
  const int j = (int)(threadIdx.x & 31u);
  if (j == 0) {
    int n = 0;
    if (on && self_word != NO_WORD && any_prim(d, key) == UNDECIDED)
      any_children(d, key, [&](u64 c, int) {
        if (n < MAXCHILD) lds.child[n] = c;
        n++;
      });
    lds.n = n < MAXCHILD ? n : MAXCHILD;
  }
  __syncthreads();
  const int n = lds.n;
  const u64 child = j < n ? lds.child[j] : EMPTY_KEY;
  __syncthreads();  // the row is rewritten by the caller's next key
  const uint32_t w = j < n ? wf(d, child) : NO_WORD;
  // this group's half of the wave's ballots
  const int sh = (int)(__lane_id() & 32u);
  auto half = [&](bool p) { return (uint32_t)(__ballot(p) >> sh); };
  const bool in = j < n;
  const uint32_t miss = half(in && w == NO_WORD);
  const uint32_t loss = half(in && w != NO_WORD && (w & 3u) == LOSS);
  const uint32_t tie = half(in && w != NO_WORD && (w & 3u) == TIE);
  const uint32_t draw = half(in && w != NO_WORD && (w & 3u) == DRAW);
  const int pv = loss ? WIN : tie ? TIE : draw ? DRAW : LOSS;
  u64 score = in ? move_score(pv, w, j) : ~0ull;
  uint32_t rmax = in && w != NO_WORD ? (w >> 2) : 0u;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const u64 so = __shfl_xor(score, o);
    const uint32_t ro = __shfl_xor(rmax, o);
    score = so < score ? so : score;
    rmax = ro > rmax ? ro : rmax;
  }
  int best = -1;
  uint32_t reduced = NO_WORD;
  if (n > 0 && !miss && score != ~0ull) {
    best = (int)(score & 31u);
    // WIN: the best child's remoteness is the smallest LOSS remoteness
    reduced = pv == WIN ? make_word(WIN, (uint32_t)(score >> 5) + 1u) : make_word(pv, rmax + 1u);
  }
  *n_out = n;
  *child_out = child;
  *word_out = w;
  *best_out = best;
  *reduced_out = reduced;
}

// ---------------------------------------------------------------------------
// k_moves: children, their words and the best move of a batch of keys
// ---------------------------------------------------------------------------
// One thread per key.  (The A/B partner gave a group of 32 lanes to each key
// -- lane 0 enumerating into LDS, the lanes fetching the children's words in
// parallel, the best move by ballot / shuffle, rows stored coalesced -- and
// took 4.74 ms against 1.30 ms for this form on the RANKED toot 4x4 table,
// all 3,468,773 positions: with ~5 children per key most of a group idled
// behind its enumerating lane.  DESIGN.md section 7c.)
template <class WF>
__global__ __launch_bounds__(256) void k_moves(Desc d, WF wf, const u64* __restrict__ keys, u64 n,
                                               u64* __restrict__ children, uint32_t* __restrict__ words,
                                               uint8_t* __restrict__ nchild, int8_t* __restrict__ best) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    const u64 key = keys[i];
    u64* cr = children + i * MAXCHILD;
    uint32_t* wr = words + i * MAXCHILD;
    int nc = 0;
    MoveAcc acc;
    if (wf(d, key) != NO_WORD && any_prim(d, key) == UNDECIDED)
      any_children(d, key, [&](u64 c, int) {
        if (nc < MAXCHILD) {
          const uint32_t w = wf(d, c);
          cr[nc] = c;
          wr[nc] = w;
          acc.add(w);
          nc++;
        }
      });
    int b = -1;
    const uint32_t red = nc ? acc.word() : NO_WORD;
    if (red != NO_WORD) {
      u64 bs = ~0ull;
      for (int j = 0; j < nc; j++) {
        const u64 sc = move_score((int)(red & 3u), wr[j], j);
        if (sc < bs) bs = sc;
      }
      b = (int)(bs & 31u);
    }
    for (int j = nc; j < MAXCHILD; j++) {
      cr[j] = EMPTY_KEY;
      wr[j] = NO_WORD;
    }
    nchild[i] = (uint8_t)nc;
    best[i] = (int8_t)b;
  }
}
// ---------------------------------------------------------------------------
// k_line: the optimal line from one key, one wave, one launch
// ---------------------------------------------------------------------------
// Both halves of the wave walk the same line (group_moves is a half-wave
// routine); the lower half writes.  *count = entries written (<= cap).
template <class WF>
__global__ __launch_bounds__(64) void k_line(Desc d, WF wf, u64 key, u64* __restrict__ keys,
                                             uint32_t* __restrict__ words, u64 cap, u64* __restrict__ count) {
  __shared__ GroupLDS lds[2];
  const int grp = (int)(threadIdx.x >> 5);
  uint32_t self = wf(d, key);
  u64 m = 0;
  while (self != NO_WORD && m < cap) {
    if (threadIdx.x == 0) {
      keys[m] = key;
      words[m] = self;
    }
    m++;
    int nc, b;
    u64 c;
    uint32_t w, red;
    group_moves(d, wf, true, key, self, lds[grp], &nc, &c, &w, &b, &red);
    if (b < 0) break;  // primitive (or a table with a hole below this position)
    key = __shfl(c, b, 32);
    self = __shfl(w, b, 32);
  }
  if (threadIdx.x == 0) *count = m;
}

// ---------------------------------------------------------------------------
// k_audit: every stored word against the reduction of its children's words
// ---------------------------------------------------------------------------
// (the layout's position enumerator and "word of key" functor, gm_table.h)
// acc[0..3]: positions, edges, mismatches, the cursor of `bad` (mismatching
// keys appended, the first `cap` kept).  Reads the table only.
template <class EN, class WF>
__global__ __launch_bounds__(256) void k_audit(Desc d, EN en, WF wf, u64* __restrict__ bad, u64 cap,
                                               u64* __restrict__ acc) {
  u64 npos = 0, edges = 0, mism = 0;
  const u64 items = en.items();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (u64)gridDim.x * blockDim.x)
    en.visit(d, i, [&](u64 key) {
      npos++;
      const uint32_t stored = wf(d, key);
      const int p = any_prim(d, key);
      uint32_t want;
      if (p != UNDECIDED) {
        want = make_word(p, 0);  // process.py:120-123: primitive, remoteness 0
      } else {
        int nch;
        want = reduce_children(d, wf, key, &nch);
        edges += (u64)nch;
      }
      if (stored == NO_WORD || stored != want) {
        mism++;
        const u64 k = atomicAdd(&acc[3], 1ull);
        if (k < cap) bad[k] = key;
      }
    });
  block_add(&acc[0], npos);
  block_add(&acc[1], edges);
  block_add(&acc[2], mism);
}

// ---------------------------------------------------------------------------
// host: the three ABI calls' bodies
// ---------------------------------------------------------------------------
static int moves_run(gm_solver* s, const uint64_t* keys_dev, uint64_t n, uint64_t* children_dev, uint32_t* words_dev,
                     uint8_t* nchild_dev, int8_t* best_dev) {
  const int grid = (int)std::min<u64>((n + kBlock - 1) / kBlock, (u64)s->grid);
  moves_words_dispatch(s, [&](auto wf) {
    hipLaunchKernelGGL(k_moves<decltype(wf)>, dim3(grid), dim3(256), 0, s->stream, s->d, wf, (const u64*)keys_dev, n,
                       (u64*)children_dev, words_dev, nchild_dev, best_dev);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

static int line_run(gm_solver* s, uint64_t key, uint64_t* keys_dev, uint32_t* words_dev, uint64_t cap, uint64_t* n) {
  u64* count = s->st->ck;
  HIPCHK(hipMemsetAsync(count, 0, sizeof(u64), s->stream));
  moves_words_dispatch(s, [&](auto wf) {
    hipLaunchKernelGGL(k_line<decltype(wf)>, dim3(1), dim3(64), 0, s->stream, s->d, wf, (u64)key, (u64*)keys_dev,
                       words_dev, (u64)cap, count);
  });
  HIPCHK(hipGetLastError());
  u64 got = 0;
  HIPCHK(hipMemcpyAsync(&got, count, sizeof got, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n = got;
  return 0;
}

static int audit_run(gm_solver* s, uint64_t* bad_keys_dev, uint64_t cap, uint64_t out[4]) {
  u64* acc = s->st->ck;
  HIPCHK(hipMemsetAsync(acc, 0, 4 * sizeof(u64), s->stream));
  moves_words_dispatch(s, [&](auto wf) {
    moves_enum_dispatch(s, [&](auto en) {
      hipLaunchKernelGGL((k_audit<decltype(en), decltype(wf)>), dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, en, wf,
                         (u64*)bad_keys_dev, (u64)cap, acc);
    });
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, acc, 4 * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  out[3] = std::min<u64>(out[3], cap);
  return 0;
}

}  // extern "C++"
