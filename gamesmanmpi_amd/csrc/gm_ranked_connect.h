// gm_ranked_connect.h -- RANKED layout (GM_MODE_RANKED) of connect four
// (games/connect_four.py, K_CONNECT): positions at COMPUTED indices, as
// gm_ranked.h does for toot-and-otto, without hands.  Planned on request only
// (GM_F_RANKED); included by gm_solver.hip after gm_ranked.h, whose rk_spread,
// packed reduction type and launch helpers it shares.
//
// A position is, per column x, its height h_x in [0, H] and the colours of
// its stack, bit y = 1 for an X piece (X moves first: at even levels).  The
// level is L = sum h_x, the mover its parity, and a stack pattern is a
// position iff it holds ceil(L / 2) X pieces.
//
// Index space: the height vectors of one level in ascending code order
// (hvcode = sum h_x (H+1)^x), each a BLOCK of 2^L slots addressed by the
// stacks' L bits concatenated column after column (column x at bits
// [off_x, off_x + h_x), off_x = sum_{c<x} h_c); the levels one after another,
// each padded to 512 slots.  One byte of word per slot (value |
// remoteness << 2, remoteness <= 30) plus a reach, an "expandable" and a
// primitive bit: 11 bits a slot.  6x5: (2^6 - 1)^6 = 6.25e10 slots, 86 GB.
//
// Addresses.  The widest levels of 6x5 and 5x6 hold more than 2^32 slots, so
// no 32-bit offset names a slot of a level.  All blocks of a level have the
// same size, so the tables name a child / parent block by its ORDINAL in its
// level (u32) and a block's first slot is the 64-bit sum lvstart[L +- 1] +
// (ordinal << (L +- 1)); inside a block a slot is its stack bits (< 2^30).
// Every board takes this one path.
//
// A move in column x: child block = hvcode + (H+1)^x, child stack bits = the
// parent's with the mover's colour bit inserted at off_x + h_x.  Forward,
// level L (pull): the board pass writes every slot's primitive value (or
// UNDECIDED) into its word byte and its primitive bit; a slot is reached iff
// it is balanced and one of its parents -- remove the top piece of a column
// whose top has the colour that moved into level L -- is expandable.
// Backward, level L: the expandable slots gather their children's words and
// apply the reference reduction (_res_red / _remote_red) -- the same words,
// counts and fingerprint as the keyed layouts
// (tests/test_gpu_connect_four_ranked.py).
extern "C++" {

// the X / O planes (the key, gm_games.h) of a board from its stacks.  C > H:
// a column's h <= H bits land on cells x + C y by one multiply (bit y times
// 2^((C-1) y) sits at C y; the shifted copies do not overlap as C - 1 >= H),
// else a loop.
__device__ __forceinline__ u64 c4_board_key(const C4Geom& g, uint32_t ph, uint32_t bits) {
  uint32_t off = 0;
  u64 xs = 0, os = 0;
  if (g.spread) {
    uint32_t x32 = 0, o32 = 0;
#pragma unroll
    for (int x = 0; x < kRankMaxCols; x++) {
      if (x >= (int)g.C) break;
      const uint32_t h = (ph >> (4 * x)) & 15u, full = (1u << h) - 1u;
      const uint32_t col = (bits >> off) & full;
      off += h;
      x32 |= ((col * g.mul) & g.msk) << x;
      o32 |= (((~col & full) * g.mul) & g.msk) << x;
    }
    xs = x32;
    os = o32;
  } else {
    for (uint32_t x = 0; x < g.C; x++) {
      const uint32_t h = (ph >> (4 * x)) & 15u, col = (bits >> off) & ((1u << h) - 1u);
      off += h;
      for (uint32_t y = 0; y < h; y++) {
        const u64 cell = 1ull << (g.C * y + x);
        if ((col >> y) & 1u) xs |= cell;
        else os |= cell;
      }
    }
  }
  return xs | (os << g.A);
}

// key -> slot (false: overlapping planes, a piece over a gap, unbalanced
// colours, bits above 2A).  Host and device share this body: on the host
// g.lvstart / g.ord are c4_shape's vectors (gm_ranked_slots), on the device
// the solver's copies.
GM_HD bool c4_slot_of(const C4Geom& g, u64 key, u64* slot, uint32_t* level) {
  const uint32_t A = g.A;
  const u64 full = (1ull << A) - 1;
  if (key >> (2 * A)) return false;
  const u64 xs = key & full, os = (key >> A) & full;
  if (xs & os) return false;
  uint32_t hv = 0, pat = 0, L = 0;
  for (uint32_t x = 0; x < g.C; x++) {
    uint32_t h = 0;
    while (h < g.H && (((xs | os) >> (g.C * h + x)) & 1)) h++;
    for (uint32_t y = h; y < g.H; y++)
      if (((xs | os) >> (g.C * y + x)) & 1) return false;  // a gap under a piece
    for (uint32_t y = 0; y < h; y++) pat |= (uint32_t)((xs >> (g.C * y + x)) & 1) << (L + y);
    hv += h * g.stride[x];
    L += h;
  }
  if ((uint32_t)__builtin_popcount(pat) != (L + 1) / 2) return false;  // X has moved ceil(L / 2) times
  *slot = g.lvstart[L] + ((u64)g.ord[hv] << L) + pat;
  *level = L;
  return true;
}

// F0: every slot of level L: the game's primitive value of its board, or
// UNDECIDED, into its word byte (remoteness 0: the byte is the word of a
// primitive), and the primitive bit.  A slot with unbalanced colours is no
// position: it is marked primitive and never reached.  One thread per slot;
// a wave = one pbits word.  (nslots: the level's 512-slot padded extent,
// nreal: its slots)
template <int KIND>
__global__ __launch_bounds__(256) void k_c4_boards(Desc d, C4Geom g, uint32_t L, u64 lvstart, uint32_t lvoff,
                                                   u64 nslots, u64 nreal) {
  const uint32_t lane = threadIdx.x & 63, need = (L + 1) / 2;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < nslots; i0 += stride) {
    const u64 i = i0 + lane;
    int pr = WIN;
    if (i < nreal) {
      const uint32_t bits = (uint32_t)(i & ((1ull << L) - 1));
      if ((uint32_t)__builtin_popcount(bits) == need)
        pr = Game<KIND>::prim(d, c4_board_key(g, g.lvph[lvoff + (i >> L)], bits));
    }
    g.words[lvstart + i] = (uint8_t)pr;
    const u64 bp = __ballot(pr != UNDECIDED);
    if (lane == 0) g.pbits[(lvstart + i0) >> 6] = bp;
  }
}

// F1 (levels L >= 6): reach and expandable bits 64 slots at a time.  The
// piece that moved into level L has colour bit l (X = 1 iff L - 1 is even).
// For a column whose top sits at bit q >= 6 of the stacks, the word's slots
// all have the same top colour and their parents are 64 consecutive slots
// (one word); for q < 6 the slots with colour l at bit q have 32 consecutive
// parents, half a word, spread back to those slots (rk_spread).  The reach
// mask is ANDed with the balance mask: slots p0 + j with popcount(p0) +
// popcount(j) = ceil(L / 2).  (nwords: the level's padded extent in words --
// every bitmap word of the level is written, the padding's as 0)
__global__ __launch_bounds__(256) void k_c4_reach(C4Geom g, uint32_t L, u64 lvstart, uint32_t lvoff, u64 nwords,
                                                  u64 nreal, u64 plvstart, BlockCount* bc, DevState* st) {
  u64 npos = 0, prims = 0;
  const uint32_t l = ((L - 1) & 1u) ? 0u : 1u, need = (L + 1) / 2;
  const u64* expd64 = reinterpret_cast<const u64*>(g.expd);
  for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (u64)gridDim.x * blockDim.x) {
    const u64 b0 = w << 6;
    u64 r = 0, e = 0;
    if (b0 < nreal) {  // (nreal: whole blocks of >= 64 slots)
      const u64 blk = b0 >> L;
      const uint32_t p0 = (uint32_t)(b0 & ((1ull << L) - 1));
      const int k = (int)need - __builtin_popcount(p0);
      const u64 valid = (k >= 0 && k <= 6) ? g.eq[k] : 0ull;
      if (valid) {
        const uint32_t ph = g.lvph[lvoff + blk];
        const uint4* pp = reinterpret_cast<const uint4*>(g.lvpa + (u64)(lvoff + blk) * kRankMaxCols);
        const uint4 pa0 = pp[0], pa1 = pp[1];
        const uint32_t pao[kRankMaxCols] = {pa0.x, pa0.y, pa0.z, pa0.w, pa1.x, pa1.y, pa1.z, pa1.w};
        uint32_t off = 0;
#pragma unroll
        for (int x = 0; x < kRankMaxCols; x++) {
          if (x >= (int)g.C) break;
          const uint32_t h = (ph >> (4 * x)) & 15u;
          off += h;
          if (h == 0) continue;
          const uint32_t q = off - 1;  // the column's top piece
          const u64 pb = plvstart + ((u64)pao[x] << (L - 1));
          if (q >= 6) {
            if (((p0 >> q) & 1u) != l) continue;
            const uint32_t pp0 = (p0 & ((1u << q) - 1u)) | ((p0 >> (q + 1)) << q);
            r |= expd64[(pb + pp0) >> 6];
          } else {
            r |= rk_spread(g.expd[(pb + (p0 >> 1)) >> 5], q) << (l << q);
          }
        }
        r &= valid;
        const u64 pm = g.pbits[(lvstart + b0) >> 6];
        e = r & ~pm;
        npos += (u64)__builtin_popcountll(r);
        prims += (u64)__builtin_popcountll(r & pm);
      }
    }
    reinterpret_cast<u64*>(g.reach)[(lvstart + b0) >> 6] = r;
    reinterpret_cast<u64*>(g.expd)[(lvstart + b0) >> 6] = e;
  }
  block_count(bc, npos, 0);
  block_add(&st->prims, prims);
}

// F1 for levels L < 6 (blocks narrower than a word): one thread per slot
// (nitems: the level's padded extent, so every bitmap word of the level is
// written; nreal: its slots)
__global__ __launch_bounds__(256) void k_c4_forward(C4Geom g, uint32_t L, u64 lvstart, uint32_t lvoff, u64 nitems,
                                                    u64 nreal, u64 plvstart, BlockCount* bc, DevState* st) {
  u64 npos = 0, prims = 0;
  const uint32_t lane = threadIdx.x & 63, need = (L + 1) / 2;
  const uint32_t l = ((L - 1) & 1u) ? 0u : 1u;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < nitems; i0 += stride) {
    const u64 i = i0 + lane;
    bool reach = false, ex = false;
    if (i < nreal) {
      const u64 blk = i >> L;
      const uint32_t bits = (uint32_t)(i & ((1ull << L) - 1));
      if ((uint32_t)__builtin_popcount(bits) == need) {
        if (L == 0) {
          reach = true;  // the root
        } else {
          const uint32_t ph = g.lvph[lvoff + blk];
          const uint32_t* pao = g.lvpa + (u64)(lvoff + blk) * kRankMaxCols;
          uint32_t off = 0;
          for (uint32_t x = 0; x < g.C && !reach; x++) {
            const uint32_t h = (ph >> (4 * x)) & 15u;
            off += h;
            if (h == 0) continue;
            const uint32_t q = off - 1;
            if (((bits >> q) & 1u) != l) continue;
            const uint32_t pb = (bits & ((1u << q) - 1u)) | ((bits >> (q + 1)) << q);
            const u64 ps = plvstart + ((u64)pao[x] << (L - 1)) + pb;
            reach = ((g.expd[ps >> 5] >> (ps & 31)) & 1u) != 0;
          }
        }
        if (reach) {
          ex = g.words[lvstart + i] == UNDECIDED;
          prims += !ex;
          npos++;
        }
      }
    }
    const u64 br = __ballot(reach), be = __ballot(ex);
    if (lane == 0) {
      const u64 w = (lvstart + i0) >> 6;  // aligned: lvstart and i0 are multiples of 64
      reinterpret_cast<u64*>(g.reach)[w] = br;
      reinterpret_cast<u64*>(g.expd)[w] = be;
    }
  }
  block_count(bc, npos, 0);
  block_add(&st->prims, prims);
}

// B: the expandable slots of level L gather their children's words.  A
// workgroup takes a tile of 256 x 32 slots: each thread reads one 32-slot
// expandable word and stages that row of 32 word bytes in LDS (the reached
// primitives' bytes are already their words: the board pass wrote them), the
// workgroup lays the expandable slots' offsets out in an LDS list (exclusive
// scan of the words' popcounts), then every thread resolves list entries, two
// per pass, all their child loads issued before any reduction.  The rows
// that hold an expandable slot go back whole (two 16-B stores): no byte
// store reaches memory.
// A child's address is the 64-bit sum cstart + (ordinal << (L + 1)) + bits.
// A tile inside one height-vector block (L >= 13) reads its block's stacks
// and child ordinals once, wave-uniform, and skips its full columns -- no
// load for a move that is illegal for every slot of the tile.  Other tiles
// read them per lane; a full column then loads the child level's first byte
// (one address for every illegal move) and its word is replaced by 0 = WIN
// in 0, which changes nothing in the reduction.
__global__ __launch_bounds__(256) void k_c4_backward(C4Geom g, uint32_t L, u64 lvstart, uint32_t lvoff, u64 nwords,
                                                     u64 cstart, BlockCount* bc, DevState* st) {
  constexpr int U = 2, NC = kRankMaxCols;
  __shared__ uint16_t list[256 * 32];
  __shared__ uint4 tw[256 * 2];  // the tile's words: 32 B per tile word, in slot order
  __shared__ uint32_t wsum[4];
  u64 edges = 0;
  uint32_t err = 0;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t C = g.C, H = g.H;
  const uint32_t cbit = (L & 1u) ? 0u : 1u;  // the mover's colour: X = 1 at even levels
  const uint8_t* cw = g.words + cstart;      // level L + 1
  for (u64 t0 = (u64)blockIdx.x * 256; t0 < nwords; t0 += (u64)gridDim.x * 256) {
    const u64 wi = t0 + threadIdx.x;
    const uint32_t m = wi < nwords ? g.expd[(lvstart >> 5) + wi] : 0u;
    if (m) {
      const uint4* src = reinterpret_cast<const uint4*>(g.words + lvstart + (wi << 5));
      const uint4 v0 = src[0], v1 = src[1];
      tw[2 * threadIdx.x] = v0;
      tw[2 * threadIdx.x + 1] = v1;
    }
    // exclusive scan of the popcounts over the workgroup
    const uint32_t c = (uint32_t)__builtin_popcount(m);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o);
      if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < 4; k++) {
      if (k < wv) before += wsum[k];
      total += wsum[k];
    }
    uint32_t at = before + incl - c;
    for (uint32_t mm = m; mm; mm &= mm - 1) list[at++] = (uint16_t)(threadIdx.x * 32 + __builtin_ctz(mm));
    // one block for the whole tile: its stacks and child ordinals, read once
    const u64 tb0 = (t0 << 5) >> L;
    const bool oneblk = ((((t0 + 255) << 5) + 31) >> L) == tb0;
    uint32_t tph = 0, tcho[NC] = {};
    if (oneblk) {
      tph = g.lvph[lvoff + tb0];
      const uint4* cp = reinterpret_cast<const uint4*>(g.lvch + (u64)(lvoff + tb0) * NC);
      const uint4 c0 = cp[0], c1 = cp[1];
      tcho[0] = c0.x, tcho[1] = c0.y, tcho[2] = c0.z, tcho[3] = c0.w;
      tcho[4] = c1.x, tcho[5] = c1.y, tcho[6] = c1.z, tcho[7] = c1.w;
    }
    __syncthreads();
    auto pass = [&](auto UNIc, const uint32_t e0) {
      constexpr bool UNI = decltype(UNIc)::value;
      uint32_t wu[U][NC], nchu[U], atu[U];
      bool liveu[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint32_t e = e0 + 256u * (uint32_t)u;
        liveu[u] = e < total;
        atu[u] = list[liveu[u] ? e : e0];
        const u64 i = (t0 << 5) + atu[u];
        const uint32_t bits = (uint32_t)(i & ((1ull << L) - 1));
        uint32_t ph, cho[NC];
        if constexpr (UNI) {
          ph = tph;
#pragma unroll
          for (int x = 0; x < NC; x++) cho[x] = tcho[x];
        } else {
          const u64 blk = i >> L;
          ph = g.lvph[lvoff + blk];
          const uint4* cp = reinterpret_cast<const uint4*>(g.lvch + (u64)(lvoff + blk) * NC);
          const uint4 c0 = cp[0], c1 = cp[1];
          cho[0] = c0.x, cho[1] = c0.y, cho[2] = c0.z, cho[3] = c0.w;
          cho[4] = c1.x, cho[5] = c1.y, cho[6] = c1.z, cho[7] = c1.w;
        }
        uint32_t off = 0, ncol = 0;
#pragma unroll
        for (int x = 0; x < NC; x++) {
          wu[u][x] = 0;
          if ((uint32_t)x >= C) continue;
          const uint32_t h = (ph >> (4 * x)) & 15u, q = off + h;
          off += h;
          // the child's stacks: the mover's colour inserted at bit q
          const uint32_t cb = (bits & ((1u << q) - 1u)) | (cbit << q) | ((bits >> q) << (q + 1));
          const bool col = h < H;
          if constexpr (UNI) {
            if (col) {  // (wave-uniform)
              wu[u][x] = cw[((u64)cho[x] << (L + 1)) + cb];
              ncol++;
            }
          } else {
            const uint32_t v = cw[col ? ((u64)cho[x] << (L + 1)) + cb : 0ull];
            wu[u][x] = col ? v : 0u;
            ncol += (uint32_t)col;
          }
        }
        nchu[u] = liveu[u] ? ncol : 0u;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        // reference-canonical _res_red / _remote_red over the children (an
        // absent child is 0: WIN in 0, changes none of the four), two
        // columns side by side in the 16-bit halves of one register, as
        // k_rk_backward (gm_ranked.h):
        //   t = (v ^ 1) & 3 -- LOSS 0, WIN 1, DRAW 2, TIE 3;
        //   min of w + (t << 8): below 256 iff a child is a LOSS, then the
        //       smallest LOSS child's word;  max of w: the largest remoteness
        rk_u16x2 mn = {0xFFFFu, 0xFFFFu}, mx = {0, 0}, pr = {0, 0};
#pragma unroll
        for (int x = 0; x < NC; x += 2) {
          const uint32_t p = wu[u][x] | (wu[u][x + 1] << 16);
          const uint32_t t = (p ^ 0x00010001u) & 0x00030003u;
          mn = __builtin_elementwise_min(mn, __builtin_bit_cast(rk_u16x2, p + (t << 8)));
          mx = __builtin_elementwise_max(mx, __builtin_bit_cast(rk_u16x2, p));
          pr = __builtin_elementwise_max(pr, __builtin_bit_cast(rk_u16x2, t));
        }
        const uint32_t mn1 = min((uint32_t)mn.x, (uint32_t)mn.y), mx1 = max((uint32_t)mx.x, (uint32_t)mx.y);
        const uint32_t pr1 = max((uint32_t)pr.x, (uint32_t)pr.y);
        if (!liveu[u]) continue;
        if (nchu[u] == 0) err |= ERR_NO_MOVES;
        edges += nchu[u];
        const uint32_t word = mn1 < 256u ? make_word(WIN, (mn1 >> 2) + 1)
                                         : make_word(pr1 == 3u ? TIE : pr1 == 2u ? DRAW : LOSS, (mx1 >> 2) + 1);
        reinterpret_cast<uint8_t*>(tw)[atu[u]] = (uint8_t)word;
      }
    };
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += 256u * U) {
      if (oneblk) pass(std::true_type(), e0);
      else pass(std::false_type(), e0);
    }
    __syncthreads();
    if (m) {  // the tile's rows with an expandable slot, whole
      uint4* dst = reinterpret_cast<uint4*>(g.words + lvstart + (wi << 5));
      dst[0] = tw[2 * threadIdx.x];
      dst[1] = tw[2 * threadIdx.x + 1];
    }
    __syncthreads();  // the list and the rows are rewritten by the next tile
  }
  if (err) atomicOr(&st->err, err);
  block_count(bc, 0, edges);
}

// the end of a solve: the root's word, then the counts (fill_red_body)
__global__ __launch_bounds__(1024) void k_c4_finish(C4Geom g, u64 root_slot, DevState* st, const BlockCount* bc) {
  if (threadIdx.x == 0)
    st->root_word = ((g.reach[root_slot >> 5] >> (root_slot & 31)) & 1u) ? (uint32_t)g.words[root_slot] : NO_WORD;
  __syncthreads();
  fill_red_body(st, bc);
}

// word of `key` at its computed slot (NO_WORD if unreached or no position):
// C4Words (gm_table.h)
__device__ __forceinline__ uint32_t c4_word(const C4Geom& g, u64 key) {
  u64 s;
  uint32_t L, w = NO_WORD;
  if (c4_slot_of(g, key, &s, &L) && ((g.reach[s >> 5] >> (s & 31)) & 1u)) w = g.words[s];
  return w;
}

// key of slot `slot` of level L (C4Enum, gm_table.h)
__device__ __forceinline__ u64 c4_slot_key(const C4Geom& g, uint32_t L, u64 slot) {
  const u64 i = slot - g.lvstart[L];
  return c4_board_key(g, g.lvph[g.lvoff[L] + (i >> L)], (uint32_t)(i & ((1ull << L) - 1)));
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct C4Shape {
  C4Geom g;
  std::vector<uint32_t> ord;            // per hvcode: its block's ordinal in its level
  std::vector<uint32_t> lvph;           // packed heights, level by level
  std::vector<uint32_t> lvch, lvpa;     // per entry: child / parent block ordinals (C4Geom)
  std::vector<uint32_t> lvoff;          // per level: first entry (T + 1)
  std::vector<u64> lvstart, lvitems;    // per level: first slot (T + 1), slots
  u64 words_off, reach_off, expd_off, pbits_off, table_bytes;
};

// why the descriptor has no RANKED layout of this kind (nullptr: it has one)
static const char* c4_rank_why(const Desc* d) {
  if (d->kind != K_CONNECT) return "game has no ranked layout";
  if (d->bsym) return "board_symmetry=1 has no ranked layout: the RANKED index has no representative form";
  if (d->L < 1 || d->L > kRankMaxCols || d->H < 1 || d->H > 7 || d->L * d->H > 30)
    return "connect four: the ranked layout takes boards of at most 8 columns, 7 rows and 30 cells";
  if ((int)d->max_levels != d->L * d->H + 1) return "connect four: the ranked layout has one level per piece count";
  double n = 1;
  for (int x = 0; x < d->L; x++) n *= (double)((2u << d->H) - 1);
  if (n > (double)(1ull << 36)) return "connect four: a ranked index space of more than 2^36 slots";
  return nullptr;
}

// (the descriptor passed c4_rank_why)
static void c4_shape(const Desc* d, C4Shape* cs) {
  C4Geom& g = cs->g;
  memset(&g, 0, sizeof g);
  g.C = (uint32_t)d->L;
  g.H = (uint32_t)d->H;
  g.R = g.H + 1;
  g.A = g.C * g.H;
  g.T = g.A + 1;
  g.spread = g.C > g.H;
  for (uint32_t y = 0; y < g.H && g.spread; y++) {
    g.mul |= 1u << ((g.C - 1) * y);
    g.msk |= 1u << (g.C * y);
  }
  uint32_t nhv = 1;
  for (uint32_t x = 0; x < g.C; x++) {
    g.stride[x] = nhv;
    nhv *= g.R;
  }
  for (int c = 0; c < 7; c++) {
    u64 m = 0;
    for (int j = 0; j < 64; j++)
      if (__builtin_popcount((unsigned)j) == c) m |= 1ull << j;
    g.eq[c] = m;
  }
  std::vector<std::vector<uint32_t>> byl(g.T);
  for (uint32_t c = 0; c < nhv; c++) {
    uint32_t s = 0, v = c;
    for (uint32_t x = 0; x < g.C; x++) {
      s += v % g.R;
      v /= g.R;
    }
    byl[s].push_back(c);  // ascending code order
  }
  cs->ord.assign(nhv, 0);
  cs->lvph.clear();
  std::vector<uint32_t> lvhv;
  cs->lvoff.assign(g.T + 1, 0);
  cs->lvstart.assign(g.T + 1, 0);
  cs->lvitems.assign(g.T, 0);
  u64 at = 0;
  for (uint32_t L = 0; L < g.T; L++) {
    cs->lvoff[L] = (uint32_t)lvhv.size();
    cs->lvstart[L] = at;
    for (size_t j = 0; j < byl[L].size(); j++) {
      const uint32_t c = byl[L][j];
      cs->ord[c] = (uint32_t)j;
      uint32_t ph = 0, v = c;
      for (uint32_t x = 0; x < g.C; x++) {
        ph |= (v % g.R) << (4 * x);
        v /= g.R;
      }
      lvhv.push_back(c);
      cs->lvph.push_back(ph);
    }
    cs->lvitems[L] = (u64)byl[L].size() << L;
    at += (cs->lvitems[L] + 511) & ~511ull;
  }
  cs->lvoff[g.T] = (uint32_t)lvhv.size();
  cs->lvstart[g.T] = at;
  cs->lvch.assign(lvhv.size() * kRankMaxCols, 0xFFFFFFFFu);
  cs->lvpa.assign(lvhv.size() * kRankMaxCols, 0xFFFFFFFFu);
  for (size_t j = 0; j < lvhv.size(); j++)
    for (uint32_t x = 0; x < g.C; x++) {
      const uint32_t h = (cs->lvph[j] >> (4 * x)) & 15u;
      if (h < g.H) cs->lvch[j * kRankMaxCols + x] = cs->ord[lvhv[j] + g.stride[x]];
      if (h > 0) cs->lvpa[j * kRankMaxCols + x] = cs->ord[lvhv[j] - g.stride[x]];
    }
  g.nslots = at;
  cs->words_off = 0;
  cs->reach_off = rup256(at);
  cs->expd_off = cs->reach_off + rup256(at / 8);
  cs->pbits_off = cs->expd_off + rup256(at / 8);
  cs->table_bytes = cs->pbits_off + rup256(at / 8);
}

// the shape's own vectors as the geometry's tables (c4_slot_of on the host)
static void c4_host_geom(C4Shape* cs) {
  cs->g.lvstart = cs->lvstart.data();
  cs->g.lvoff = cs->lvoff.data();
  cs->g.ord = cs->ord.data();
  cs->g.lvph = cs->lvph.data();
  cs->g.lvch = cs->lvch.data();
  cs->g.lvpa = cs->lvpa.data();
}

static int plan_c4_ranked(const Desc* d, uint64_t max_table_bytes, gm_plan_t* out, bool* fits) {
  C4Shape cs;
  c4_shape(d, &cs);
  *fits = max_table_bytes == 0 || cs.table_bytes <= max_table_bytes;
  out->mode = GM_MODE_RANKED;
  out->table_slots = cs.g.nslots;
  out->table_bytes = cs.table_bytes;
  out->level_capacity = 1;
  out->scratch_bytes = scratch_bytes_for(d->max_levels);
  out->max_levels = (uint32_t)d->max_levels;
  return 0;
}

static int c4_setup(gm_solver* s, const gm_buffers* buf) {
  C4Shape cs;
  c4_shape(&s->d, &cs);
  if (buf->table_bytes < cs.table_bytes)
    return fail(GM_EINVAL, "ranked table of %llu bytes, the plan needs %llu", (unsigned long long)buf->table_bytes,
                (unsigned long long)cs.table_bytes);
  C4Geom& g = cs.g;
  char* t = (char*)buf->table;
  g.words = (uint8_t*)(t + cs.words_off);
  g.reach = (uint32_t*)(t + cs.reach_off);
  g.expd = (uint32_t*)(t + cs.expd_off);
  g.pbits = (u64*)(t + cs.pbits_off);
  // the index tables: an allocation of the solver's own, so that the table
  // buffer holds nothing a solve does not write
  const size_t T1 = g.T + 1, nhv = cs.ord.size(), ne = cs.lvph.size();
  const size_t o_off = rup256(T1 * 8), ord_off = o_off + rup256(T1 * 4), ph_off = ord_off + rup256(nhv * 4);
  const size_t ch_off = ph_off + rup256(ne * 4), pa_off = ch_off + rup256(ne * 4 * kRankMaxCols);
  const size_t bytes = pa_off + rup256(ne * 4 * kRankMaxCols);
  if (!s->c4_dev) HIPCHK(hipMalloc(&s->c4_dev, bytes));
  char* dv = (char*)s->c4_dev;
  HIPCHK(hipMemcpy(dv, cs.lvstart.data(), T1 * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dv + o_off, cs.lvoff.data(), T1 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dv + ord_off, cs.ord.data(), nhv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dv + ph_off, cs.lvph.data(), ne * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dv + ch_off, cs.lvch.data(), ne * 4 * kRankMaxCols, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dv + pa_off, cs.lvpa.data(), ne * 4 * kRankMaxCols, hipMemcpyHostToDevice));
  g.lvstart = (const u64*)dv;
  g.lvoff = (const uint32_t*)(dv + o_off);
  g.ord = (const uint32_t*)(dv + ord_off);
  g.lvph = (const uint32_t*)(dv + ph_off);
  g.lvch = (const uint32_t*)(dv + ch_off);
  g.lvpa = (const uint32_t*)(dv + pa_off);
  s->kg = g;
  s->rlvoff = cs.lvoff;
  s->rlvstart = cs.lvstart;
  s->rlvitems = cs.lvitems;
  return 0;
}

using RankedConnectKinds = KindList<K_CONNECT_5x4, K_CONNECT_6x5, K_CONNECT>;  // by fixed_kind

// one forward level: the board pass, then reach / counts
static void c4_forward_level(gm_solver* s, hipStream_t st, uint32_t L) {
  const C4Geom& g = s->kg;
  const u64 n = s->rlvstart[L + 1] - s->rlvstart[L];  // 512-padded: every byte and bitmap word written
  const u64 pl = L ? s->rlvstart[L - 1] : 0;
  kind_dispatch<RankedConnectKinds>(fixed_kind(s->d), [&](auto KC) {
    hipLaunchKernelGGL((k_c4_boards<decltype(KC)::value>), dim3(rank_grid(s, n)), dim3(256), 0, st, s->d, g, L,
                       s->rlvstart[L], s->rlvoff[L], n, s->rlvitems[L]);
  });
  if (L >= 6)
    hipLaunchKernelGGL(k_c4_reach, dim3(rank_grid(s, n / 64)), dim3(256), 0, st, g, L, s->rlvstart[L], s->rlvoff[L],
                       n / 64, s->rlvitems[L], pl, s->bcount, s->st);
  else
    hipLaunchKernelGGL(k_c4_forward, dim3(rank_grid(s, n)), dim3(256), 0, st, g, L, s->rlvstart[L], s->rlvoff[L], n,
                       s->rlvitems[L], pl, s->bcount, s->st);
}

static void c4_backward_level(gm_solver* s, hipStream_t st, uint32_t L) {
  const u64 nw = (s->rlvitems[L] + 31) / 32;  // 32-slot tile words
  hipLaunchKernelGGL(k_c4_backward, dim3(rank_grid(s, nw)), dim3(256), 0, st, s->kg, L, s->rlvstart[L], s->rlvoff[L],
                     nw, s->rlvstart[std::min<uint32_t>(L + 1, s->kg.T)], s->bcount, s->st);
}

static void c4_finish(gm_solver* s, hipStream_t st) {
  hipLaunchKernelGGL(k_c4_finish, dim3(1), dim3(1024), 0, st, s->kg, s->rlvstart[0], s->st,
                     (const BlockCount*)s->bcount);
}

}  // extern "C++"
