// gm_sym.h -- board symmetries as key maps (params "board_symmetry=1").
//
// A symmetric table stores, for every orbit of the game's board group, the
// orbit's smallest key.  Only the cell planes move: hands, turn bit, pass
// count and side to move stay where they are, so every map keeps the level,
// the primitive value and the child count of a position.  The maps are
// branch-free bit permutations built from delta swaps
//     t = (k ^ (k >> s)) & m;  k ^= t ^ (t << s)
// (exchange the bits of m with the bits s above them) and bit reversal: they
// run once per emitted child in the expand kernels and once per key in every
// lookup (query, moves, audit, census, export).  One GM_HD body serves the
// kernels and the host (gm_symmetry, gm_host_expand).
//
// Groups, in the order gm_symmetry(which = i) numbers them (identity
// excluded; include/gamesman.h):
//   tic-tac-toe (18-bit key, 2 bits per cell, cell 3x+y), all 8 maps of the
//     square.  R: x -> 2-x, C: y -> 2-y, T: (x,y) -> (y,x), applied right to
//     left:  0 R   1 C   2 RC   3 T   4 RT   5 CT   6 RCT
//   toot-and-otto (any board): 0 the left-right mirror x -> L-1-x of both
//     planes, floor(L/2) delta swaps whose masks cover the 2H rows of the
//     T and O planes at once (constexpr in TootFixed<L,H>::mirror, Desc::mir
//     for the generic form)
//   connect four (any board): 0 the same mirror of its X and O planes, with
//     the same masks (ConnectFixed<L,H,K>::mirror, Desc::mir)
//   othello LxL, the maps that keep the colours of the start position:
//     0 the 180-degree turn (bit reversal of each A-bit plane)
//     1 the transpose       2 the anti-transpose (turn of the transpose)
//     L = 4 transposes both planes with the two-step delta-swap transpose;
//     L = 2 uses the per-cell form (sym_oth_transpose_cells, written for any
//     L).  L = 3 and 5 are refused when the descriptor is built: the module
//     places their start position off centre (float coordinates truncated),
//     the transpose moves it, and a map that moves the root is not accepted.
#pragma once
#include <stdint.h>

namespace gm {

GM_HD uint64_t sym_dswap(uint64_t k, uint64_t m, int s) {
  const uint64_t t = (k ^ (k >> s)) & m;
  return k ^ t ^ (t << s);
}
GM_HD uint64_t sym_min(uint64_t a, uint64_t b) { return b < a ? b : a; }
GM_HD uint64_t sym_brev64(uint64_t v) {
#if defined(__clang__)
  return __builtin_bitreverse64(v);
#else
  v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
  v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
  v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
  return __builtin_bswap64(v);
#endif
}

// ---- tic-tac-toe ----------------------------------------------------------
// rows are 6 bits (x), cells 2 bits (y) inside them
GM_HD uint64_t sym_ttt_R(uint64_t k) { return sym_dswap(k, 0x3Full, 12); }    // row 0 <-> row 2
GM_HD uint64_t sym_ttt_C(uint64_t k) { return sym_dswap(k, 0x30C3ull, 4); }   // cell 0 <-> cell 2 of every row
GM_HD uint64_t sym_ttt_T(uint64_t k) {
  k = sym_dswap(k, 0xC0Cull, 4);  // cells 1 <-> 3 and 5 <-> 7
  return sym_dswap(k, 0x30ull, 8);  // cells 2 <-> 6
}
constexpr int kSymTttMaps = 7;
GM_HD uint64_t sym_ttt_map(uint64_t k, int which) {
  const int w = which + 1;  // bit 0: R, bit 1: C, bit 2: T (T first)
  if (w & 4) k = sym_ttt_T(k);
  if (w & 2) k = sym_ttt_C(k);
  if (w & 1) k = sym_ttt_R(k);
  return k;
}
GM_HD uint64_t sym_ttt_canon(uint64_t k) {
  // the four images without the transpose, then the same four of T(k)
  const uint64_t r = sym_ttt_R(k), c = sym_ttt_C(k), rc = sym_ttt_C(r);
  const uint64_t t = sym_ttt_T(k), tr = sym_ttt_R(t), tc = sym_ttt_C(t), trc = sym_ttt_C(tr);
  return sym_min(sym_min(sym_min(k, r), sym_min(c, rc)), sym_min(sym_min(t, tr), sym_min(tc, trc)));
}

// ---- toot-and-otto --------------------------------------------------------
constexpr int kSymMaxMirror = 12;  // floor(L / 2) for L <= 25
// bit i of each of the 2H rows of L bits (both planes)
constexpr uint64_t sym_toot_mask(int L, int H, int i) {
  uint64_t m = 0;
  for (int r = 0; r < 2 * H; r++) m |= 1ull << (L * r + i);
  return m;
}
GM_HD uint64_t sym_toot_mirror(const Desc& d, uint64_t k) {
  for (int i = 0; i < d.nmir; i++) k = sym_dswap(k, d.mir[i], d.L - 1 - 2 * i);
  return k;
}
GM_HD uint64_t sym_toot_canon(const Desc& d, uint64_t k) { return sym_min(k, sym_toot_mirror(d, k)); }
template <int L, int H, int I = 0>
GM_HD uint64_t sym_toot_mirror_fixed(uint64_t k) {
  if constexpr (I < L / 2) {
    constexpr uint64_t m = sym_toot_mask(L, H, I);
    return sym_toot_mirror_fixed<L, H, I + 1>(sym_dswap(k, m, L - 1 - 2 * I));
  } else {
    return k;
  }
}

// ---- othello --------------------------------------------------------------
GM_HD uint64_t sym_oth_turn(const Desc& d, uint64_t k) {
  const int A = d.A;
  const uint64_t w = sym_brev64(k & d.full) >> (64 - A), b = sym_brev64((k >> A) & d.full) >> (64 - A);
  return (k & ~((1ull << (2 * A)) - 1)) | w | (b << A);
}
// any L: cell L*y+x <-> cell L*x+y, one cell pair at a time (reached with L = 2)
GM_HD uint64_t sym_oth_transpose_cells(const Desc& d, uint64_t k) {
  const int L = d.L, A = d.A;
  const uint64_t both = 1ull | (1ull << A);
  for (int y = 1; y < L; y++)
    for (int x = 0; x < y; x++) k = sym_dswap(k, both << (L * x + y), (L - 1) * (y - x));
  return k;
}
GM_HD uint64_t sym_oth_transpose(const Desc& d, uint64_t k) {
  if (d.L == 4) {  // both 16-bit planes at once
    k = sym_dswap(k, 0x0A0A0A0Aull, 3);
    return sym_dswap(k, 0x00CC00CCull, 6);
  }
  return sym_oth_transpose_cells(d, k);
}
constexpr int kSymOthMaps = 3;
GM_HD uint64_t sym_oth_map(const Desc& d, uint64_t k, int which) {
  if (which == 0) return sym_oth_turn(d, k);
  const uint64_t t = sym_oth_transpose(d, k);
  return which == 1 ? t : sym_oth_turn(d, t);
}
GM_HD uint64_t sym_oth_canon(const Desc& d, uint64_t k) {
  const uint64_t t = sym_oth_transpose(d, k);
  return sym_min(sym_min(k, sym_oth_turn(d, k)), sym_min(t, sym_oth_turn(d, t)));
}

// ---- any game -------------------------------------------------------------
// (the number of maps per kind: Game<K>::kMaps, sym_board_maps in gm_games.h)
GM_HD uint64_t sym_board_map(const Desc& d, uint64_t k, int which) {
  if (d.kind == K_TTT) return sym_ttt_map(k, which);
  if (d.kind == K_TOOT || d.kind == K_CONNECT) return sym_toot_mirror(d, k);
  return sym_oth_map(d, k, which);
}
// the orbit's representative: the smallest image
GM_HD uint64_t sym_board_canon(const Desc& d, uint64_t k) {
  if (d.kind == K_TTT) return sym_ttt_canon(k);
  if (d.kind == K_TOOT || d.kind == K_CONNECT) return sym_toot_canon(d, k);
  return sym_oth_canon(d, k);
}

}  // namespace gm
