// gm_solver.hip -- tier-synchronous retrograde solver for gfx950 (MI355X)
// behind the C-ABI of include/gamesman.h.  The library is ONE translation
// unit: this file holds what every layout shares and the C-ABI, and includes
// the layouts' kernels and host paths in this order:
//
//   gm_codec.h gm_games.h gm_md5.h  keys, the games' moves, md5 owners
//   gm_plane.h           PLANES kernels
//   (here)               errors, SolveEvents, gm_registry.h (host), the dense /
//                        halo / group / column geometry, DevState, the HASHED
//                        kernels (k_seed, k_expand, k_finalize, k_resolve, ...)
//   gm_dense.h           DENSE kernels
//   gm_keyed_shard.h     md5-sharded HASHED kernels (gm_ks_*)
//   gm_bucketed.h        BUCKETED kernels
//   (here)               struct gm_solver, the HASHED host path (run_hashed),
//                        the codec C-ABI, k_fill_red
//   gm_xchg.h            the shards' exchange layer: transport modes and group
//                        checks, all-gather, ranged send / receive, the
//                        end-of-solve reduction (no kernels)
//   gm_dense_run.h       DENSE host path: setup, launches, halo exchanges,
//                        run_dense (no kernels)
//   gm_plane_run.h       PLANES host path and its late kernels
//   gm_ranked.h gm_ranked_shard.h  RANKED kernels and host path, its md5 shards
//   gm_ranked_connect.h            RANKED kernels and host path of connect four
//   gm_bucketed_run.h    BUCKETED host path (no kernels)
//   gm_bucketed_shard.h  md5-sharded BUCKETED levels
//   (here)               the C-ABI over the layouts: plans, creation, solves
//   gm_table.h           the layout views (word of key, position enumerator,
//                        pair source); query, positions, checksum
//   gm_moves.h           move analysis and the table audit
//   gm_census.h          the census by value, remoteness and level
//   (here)               readers, gm_solve, gm_ks_*, the explicit-graph solve
//
// The HASHED pipeline (this file) replaces the reference's asynchronous
// per-state job machinery (src/process.py:37-267, src/job.py) with a
// level-synchronous one:
//   forward, level L = 0..T-1 (K1+K2, k_expand<G>): every position of level L
//     is tested with primitive(); the non-primitive ones generate their
//     children (gen_moves+do_move fused), which are inserted into the HBM hash
//     table by 64-bit CAS; a child inserted for the first time is appended
//     (wave-aggregated atomics) to the position store of level L+1 or L+2.
//   backward, level L = T-1..0 (K3, k_resolve<G>): each position of level L
//     re-generates its children, probes their 32-bit words and reduces them
//     with the reference-canonical rule of _res_red/_remote_red (SURVEY §8a
//     A8/A9), then stores its own word.
//
// HBM layout (caller-allocated, gamesman.h):
//   table  : gm_slot[2^k] {u64 key, u32 word, u32 spare}, open addressing,
//            linear probing, EMPTY key = ~0.  Replaces the resolved/remote
//            CacheDicts (src/cache_dict.py) -- one 16-B line per probe
//            serves both key compare and word.
//   levels : u64 keys of every reachable position grouped by level.  +1
//            children grow a stack from the front, +2 children a stack from
//            the back, so each level is at most two contiguous segments.
//   scratch: DevState (cursors, counters, error bits, per-level segments).
// No host synchronisation inside the level loops: segment bounds travel
// through device memory (k_finalize), so a whole solve is enqueued at once.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "gm_solver.hip is written for gfx950 (MI355X) only: v_bitop3_b32, v_pk_maximum3_f16 on f16 subnormals"
#endif

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include <memory>
#include <type_traits>
#include <map>
#include <thread>
#include <atomic>

#include "../../include/gamesman.h"
#include "gm_codec.h"
#include "gm_games.h"
#include "gm_md5.h"
#include "gm_plane.h"

using namespace gm;
typedef unsigned long long u64;

// A/B knobs of the measurement labs (tools/*.sh): environment variables read
// ONLY by a library built with -DGM_LAB=1 (make lab ->
// libgamesman_hip_lab.so).  In the shipped library every knob reads as unset,
// so no environment can select a timing-only variant (some of them write
// wrong words on purpose, e.g. GM_RK_DBG) or change the product's schedule.
#ifndef GM_LAB
#define GM_LAB 0
#endif
static const char* lab_env(const char* name) {
#if GM_LAB
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) return fail(GM_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

// The events made for ONE solve, destroyed on every return path.  Events
// that live with the solver (pev, pse, the ring slots') are not made here.
struct SolveEvents {
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;  // start, forward end, backward end
  std::vector<hipEvent_t> kx, kr;  // kernel timing: start / stop pairs of the forward's / backward's launches
  SolveEvents() = default;
  SolveEvents(const SolveEvents&) = delete;
  SolveEvents& operator=(const SolveEvents&) = delete;
  ~SolveEvents() {
    for (hipEvent_t e : all) (void)hipEventDestroy(e);
  }
  int make(hipEvent_t* e, unsigned flags = 0) {
    HIPCHK(hipEventCreateWithFlags(e, flags));
    all.push_back(*e);
    return 0;
  }
  // e0, e1, e2, then (pairs > 0) kx and kr of `pairs` start / stop pairs each
  int begin(size_t pairs = 0) {
    if (make(&e0) || make(&e1) || make(&e2)) return GM_EHIP;
    kx.resize(2 * pairs);
    kr.resize(2 * pairs);
    for (auto& e : kx)
      if (make(&e)) return GM_EHIP;
    for (auto& e : kr)
      if (make(&e)) return GM_EHIP;
    return 0;
  }
  // milliseconds summed over the first n pairs of kx / kr
  static int pairs_ms(const std::vector<hipEvent_t>& p, int n, double* sum) {
    *sum = 0;
    for (int i = 0; i < n; i++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, p[2 * i], p[2 * i + 1]));
      *sum += ms;
    }
    return 0;
  }

 private:
  std::vector<hipEvent_t> all;
};


// queued one-table PLANES solves (gm_solver_solve_async): a ring slot holds
// one solve's events (start, forward end, backward end, its completion --
// recorded after the counts' copy -- and the forward's start) and its counts
// in pinned host memory
constexpr int kPlaneRing = 8;
struct PlaneSlot {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // (4: the forward's start, no timing)
  u64* host = nullptr;
  double t_enq = 0;  // host clock at enqueue (ms)
  bool lite = false;  // only ev[0] and ev[3] recorded (a queued one-launch solve)
};

enum : uint32_t {
  ERR_TABLE_FULL = 1u,
  ERR_LEVELS_FULL = 2u,
  ERR_BAD_STEP = 4u,
  ERR_CHILD_MISSING = 8u,
  ERR_CHILD_UNRESOLVED = 16u,
  ERR_NO_MOVES = 32u,
  ERR_SELF_MISSING = 64u,
  // a shard failed on its host side (a deferred error: it kept serving its
  // halo transfers so that its peers finished, then reported through the
  // end-of-solve reduction; gm_plane_run.h plane_backward_staged)
  ERR_SHARD_FAILED = 512u,
  // the one-launch PLANES backward (k_plane_flow) gave up waiting for a
  // neighbour plane: the launch drained, the words are incomplete
  ERR_PLANE_STALL = 1024u,
};

#include "gm_registry.h"

// Shard geometry of a dense table.  world == 1: the whole prefix space.
// world > 1: the values [0, E) of the TOP prefix digit (heap K-1) are cut
// into blocks of B and block k is owned by rank k mod world (round robin:
// every rank's top values spread over the whole range, so the ranks'
// per-level work stays close -- DESIGN.md §Multi-GPU).  Each block keeps
// halo slices [kB-2, kB) (children: one move lowers a heap by 1 or 2) and
// [kB+B, kB+B+2) (parents, for the pull-form forward pass).  B = 8 when
// every rank gets at least two blocks, else ceil(E / world) (one block per
// rank).  The geometry is a function of (descriptor, rank, world) alone, so
// every rank derives the same halo sizes.
struct DenseGeom {
  DenseView v;
  u64 nblocks, nb;
};
static int dense_geom(const Desc* d, int rank, int world, DenseGeom* g) {
  memset(g, 0, sizeof *g);
  if (world <= 1) {
    g->v.p_lo = 0;
    g->v.p_hi = d->W;
    g->v.Wl = d->W;
    g->v.Wbl = (d->W + 63) & ~63ull;
    g->v.world = 1;
    g->v.zshift = -1;
    g->nblocks = g->nb = 1;
    return 0;
  }
  if (d->nheaps < 2) return fail(GM_EINVAL, "sharding needs at least 2 heaps");
  if (rank < 0 || rank >= world) return fail(GM_EINVAL, "bad shard %d/%d", rank, world);
  const int k = d->nheaps - 1;
  const u64 E = d->base[k], Z = d->pstride[k];
  if (Z % 64) return fail(GM_EINVAL, "shard slices must hold a multiple of 64 prefixes (got %llu)", (unsigned long long)Z);
  const u64 B = E >= 16 * (u64)world ? 8 : (E + world - 1) / world;
  const u64 nblocks = B ? (E + B - 1) / B : 0;
  if (B < 2 || nblocks < (u64)world)
    return fail(GM_EINVAL, "top heap of %llu values cannot give %d ranks blocks of >= 2", (unsigned long long)E, world);
  g->nblocks = nblocks;
  g->nb = (nblocks - (u64)rank + world - 1) / world;
  DenseView& v = g->v;
  v.blk = 1;
  v.B = (uint32_t)B;
  v.world = (uint32_t)world;
  v.rank = (uint32_t)rank;
  v.Z = Z;
  v.E = E;
  v.zshift = (Z & (Z - 1)) ? -1 : __builtin_ctzll(Z);
  v.olo = 2;
  v.ohi = (uint32_t)B + 2;
  v.Wl = g->nb * (B + 4) * Z;
  v.Wbl = v.Wl;  // multiple of 64
  if (v.Wl * 4 > 0xFFFFFFF0ull)  // the shard resolve addresses a level with 32-bit buffer offsets
    return fail(GM_EINVAL, "shard of %llu prefixes per level: more than 2^30 (use more ranks)",
                (unsigned long long)v.Wl);
  v.p_lo = 0;
  v.p_hi = v.Wl;
  return 0;
}
// word area of a dense table: 8- or 16-bit order forms when the plan chose
// them (dense_plan_bits: one-GPU K_SUM tables the 16- / 8-prefix kernels
// handle), else 32-bit
static u64 dense_words_bytes(const Desc* d, const DenseGeom& g, uint32_t wbits) {
  return ((u64)d->max_levels * g.v.Wl * (wbits / 8) + 255) & ~255ull;
}
static u64 dense_bits_bytes(const Desc* d, const DenseGeom& g) {
  return (u64)d->max_levels * g.v.Wbl / 8;
}


// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
struct LevelSeg {
  u64 fb, fe;      // front segment [fb, fe) of the level store
  u64 c2lo, c2hi;  // back segment: back-stack counts [c2lo, c2hi)
};
struct DevState {
  u64 cursor_front;
  u64 cursor_back;
  u64 edges;
  u64 prims;
  u64 max_width;
  uint32_t err;
  uint32_t root_word;
  u64 ks_cursor;    // keyed shards: children emitted by k_ks_expand
  u64 red[5];     // cross-shard reduction: positions, edges, prims, root word + 1, err
  uint32_t word_bits;  // dense: table word width of the solve in progress (resume reads it back)
  uint32_t pad_;
  u64 ck[6];        // gm_solver_checksum: checksum, positions, W, L, T, D
  LevelSeg seg[1];  // [max_levels + 2]
};
static size_t devstate_bytes(int max_levels) {
  return sizeof(DevState) + sizeof(LevelSeg) * (size_t)(max_levels + 2);
}
// Scratch = DevState (cleared per solve) + the dense mask tables (written
// once at solver creation): TS[64] then TD[16][64], u64 each.
constexpr size_t kMaskTableWords = 64 * 17;
static size_t mask_tables_offset(int max_levels) { return (devstate_bytes(max_levels) + 255) / 256 * 256; }
// then per-block position/edge counts of the octet resolves (block_count):
// one plain read-modify-write per block and launch instead of device-scope
// atomics on one line, which serialise at ~12 ns each (MI355X_MICROARCH.md
// "fanin"): 768 resident blocks x 2 counters cost ~18 us at the end of every
// launch.  Cleared per solve, summed by k_fill_red.
struct BlockCount {
  u64 npos, edges;
};
constexpr int kCountSlots = 4096;  // >= any octet-resolve grid (host clamps)
static size_t count_slots_offset(int max_levels) { return mask_tables_offset(max_levels) + kMaskTableWords * sizeof(u64); }
static size_t scratch_bytes_for(int max_levels) {
  return count_slots_offset(max_levels) + kCountSlots * sizeof(BlockCount);
}
// Packed word halos of sharded power-of-two dense tables (exchange_words):
// after the mask tables, the group offset table off[XN][G] (u32; G = Z/64
// groups of a slice, XN = values of x = S - t that leave any slot valid),
// then a send and a receive buffer of 2 slices of words each.
struct HaloGeom {
  u64 Z = 0, nb = 0;
  int XN = 0, NG = 0, NYn = 0, mj = 0, top = 0;
  bool on = false;
};
static HaloGeom halo_geom(const Desc* d, int world, u64 nb) {
  HaloGeom h;
  if (world <= 1 || !d->pow2 || d->nheaps < 3 || d->base[1] < 4) return h;
  const int k = d->nheaps - 1;
  h.Z = d->pstride[k];
  if (h.Z % 256) return h;
  h.nb = nb;
  h.top = k;
  int slow = 0;
  for (int i = 1; i < k; i++) {
    slow += (int)d->heap[i];
    h.mj += (int)((255u >> d->pshift[i]) & (d->base[i] - 1));
  }
  h.XN = slow + (int)d->heap[0] + 1;  // x = S - t with any non-hole
  h.NG = slow + 2;                    // column digit sums 0..slow, plus the total
  h.NYn = h.mj + (int)d->heap[0] + 1;
  h.on = true;
  return h;
}
// column tables PB[XN][NG], NY[NYn], CS[NG] (u32) + send and receive
// buffers of 2 slices per local block
static size_t halo_tab_bytes(const HaloGeom& h) {
  auto r = [](size_t b) { return (b + 255) / 256 * 256; };
  return r((size_t)h.XN * h.NG * 4) + r((size_t)h.NYn * 4) + r((size_t)h.NG * 4);
}
static size_t halo_bytes(const HaloGeom& h) {
  if (!h.on) return 0;
  return halo_tab_bytes(h) + 2 * (h.nb * 2 * h.Z * 4);
}

// Active-group lists of single-table power-of-two dense layouts
// (k_dense_resolve4): per level, the 256-prefix groups holding at least one
// non-hole.  A level's band (dense_band) is a loose bound -- at the narrow
// ends of the tier sequence it spans nearly the whole row while a few
// percent of its groups hold positions -- and XCD chunks of a band split the
// level's work unevenly; a launch over the list sweeps only live groups.
// Group g (base 256 g) holds digit sums [gs, gs + mj] with gs =
// digitsum(256 g), mj = digitsum(255) (pow2 digits are bit fields), so it is
// live at level L iff [gs, gs + mj] meets [S - heap0, S].
//
// Order (L2 reuse): a group's children lie in the same group or in groups
// one or two steps down one digit.  With g = column + top * C (C = groups
// per top-digit slice), the level's columns are cut into 8 contiguous
// ranges of equal live-group count, one per XCD, and each XCD walks its
// range TOP-MAJOR (all its columns at top value t, then t + 1, ...): the
// top-digit children (4-8 MB away in address order) were touched one or two
// steps earlier, the other digits' children are neighbouring columns of the
// same step -- both still in that XCD's L2.  Tables without a top digit
// above the group fall back to address order in 8 equal shares.
struct GroupGeom {
  bool on = false;
  u64 groups = 0;
  int mj = 0;
};
static GroupGeom group_geom(const Desc* d, int world) {
  GroupGeom g;
  if (world != 1 || !d->pow2 || d->nheaps < 2 || d->base[1] < 4 || d->W % 256 || d->W * 4 > 0xFFFFFFF0ull)
    return g;
  g.groups = d->W / 256;
  for (int i = 1; i < d->nheaps; i++) g.mj += (int)((255u >> d->pshift[i]) & (d->base[i] - 1));
  g.on = true;
  return g;
}
// Plan-time choice of 16-bit table words (half the HBM of the word area):
// one-GPU tables the octet kernel (k_dense_resolve8p) can solve, unless the
// plan flags ask for 32-bit words or the one-prefix kernel.  The same flags
// must reach gm_solver_create_shard (gm_buffers.flags), which sizes the
// table against them: a table planned with 16-bit words cannot be handed a
// 32-bit kernel (GM_EINVAL at creation, never a fault).
static uint32_t dense_plan_bits(const Desc* d, int world, uint32_t flags) {
  if (world != 1 || d->kind != K_SUM || !d->pow2 || d->nheaps < 2 || d->nheaps > 8 || d->base[1] < 8 ||
      d->root_sum >= 0x7FFF || d->W * 2 > 0xFFFFFFF0ull || !group_geom(d, 1).on ||
      (flags & (GM_F_WORDS32 | GM_F_RESOLVE_SCALAR)))
    return 32;
  // 8-bit words (k_dense_resolve16p): 16 prefixes per lane, every
  // remoteness < 255 (dense_parent8)
  if (d->base[1] >= 16 && d->root_sum <= 253 && !(flags & GM_F_WORDS16)) return 8;
  return 16;
}
static void group_sums(const Desc* d, const GroupGeom& g, std::vector<uint16_t>& gs) {
  gs.resize(g.groups);
  for (u64 k = 0; k < g.groups; k++) {
    int s = 0;
    for (int i = 1; i < d->nheaps; i++) s += (int)(((k * 256) >> d->pshift[i]) & (d->base[i] - 1));
    gs[k] = (uint16_t)s;
  }
}
static bool group_live(const Desc* d, const GroupGeom& g, int gs, int L) {
  const int S = (int)d->root_sum - L;
  return gs <= S && gs + g.mj >= S - (int)d->heap[0];
}
static u64 group_entries(const Desc* d, const GroupGeom& g) {
  if (!g.on) return 0;
  std::vector<uint16_t> gs;
  group_sums(d, g, gs);
  std::vector<u64> hist(1 << 16, 0);
  for (uint16_t x : gs) hist[x]++;
  u64 n = 0;
  for (int L = 0; L < d->max_levels; L++)
    for (int x = 0; x < (1 << 16); x++)
      if (hist[x] && group_live(d, g, x, L)) n += hist[x];
  return n;
}
static size_t group_bytes(const Desc* d, int world) {
  const GroupGeom g = group_geom(d, world);
  return g.on ? (group_entries(d, g) * 4 + 255) / 256 * 256 : 0;
}

// Column permutation (k_dense_resolve4c): the Z / 256 groups ("columns") of
// a top-digit slice sorted by their digit sum over the digits below the
// top; cstart[x] = first position with sum >= x.  Any world.
struct ColGeom {
  bool on = false;
  int top = 0, mj = 0, maxgs = 0;
  u64 C = 0;
};
static ColGeom col_geom(const Desc* d) {
  ColGeom c;
  if (!d->pow2 || d->nheaps < 3 || d->base[1] < 4) return c;
  c.top = d->nheaps - 1;
  const u64 Z = d->pstride[c.top];
  if (Z % 256 || Z * 4 > 0xFFFFFFF0ull) return c;
  c.C = Z / 256;
  for (int i = 1; i < c.top; i++) {
    c.mj += (int)((255u >> d->pshift[i]) & (d->base[i] - 1));
    c.maxgs += (int)d->heap[i];
  }
  c.on = true;
  return c;
}
static size_t col_bytes(const Desc* d) {
  const ColGeom c = col_geom(d);
  return c.on ? (c.C * 4 + 255) / 256 * 256 : 0;
}
static void build_colperm(const Desc* d, const ColGeom& c, std::vector<uint32_t>& perm, std::vector<uint32_t>& cstart) {
  std::vector<int> gs(c.C);
  for (u64 k = 0; k < c.C; k++) {
    int x = 0;
    for (int i = 1; i < c.top; i++) x += (int)(((k * 256) >> d->pshift[i]) & (d->base[i] - 1));
    gs[k] = x;
  }
  cstart.assign((size_t)c.maxgs + 2, 0);
  for (u64 k = 0; k < c.C; k++) cstart[(size_t)gs[k] + 1]++;
  for (size_t x = 1; x < cstart.size(); x++) cstart[x] += cstart[x - 1];
  perm.assign(c.C, 0);
  std::vector<uint32_t> at(cstart.begin(), cstart.end() - 1);
  for (u64 k = 0; k < c.C; k++) perm[at[gs[k]]++] = (uint32_t)k;  // stable: address order within a sum
}

GM_HD u64 mix64(u64 x) {  // splitmix64 finaliser (host: gm_mix64, the keyed tablebase's reader)
  x ^= x >> 31;
  x *= 0x7fb5d329728ea185ull;
  x ^= x >> 27;
  x *= 0x81dadef4bc2dd44dull;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ u64 lanemask_lt() {
  return (1ull << __lane_id()) - 1ull;
}

// Wave-aggregated append: one atomic per wave per call site.
__device__ __forceinline__ u64 wave_reserve(u64* cursor, bool pred) {
  u64 mask = __ballot(pred);
  if (mask == 0) return 0;
  int leader = __ffsll((long long)mask) - 1;
  u64 base = 0;
  if ((int)__lane_id() == leader) base = atomicAdd(cursor, (u64)__popcll(mask));
  base = __shfl(base, leader);
  return base + (u64)__popcll(mask & lanemask_lt());
}

// insert key; true iff this call created the slot
__device__ __forceinline__ bool table_insert(gm_slot* tab, u64 mask, u64 key, uint32_t* err) {
  u64 h = mix64(key) & mask;
  for (u64 probe = 0; probe <= mask; probe++) {
    u64 k = __hip_atomic_load(&tab[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return false;
    if (k == EMPTY_KEY) {
      u64 old = atomicCAS((u64*)&tab[h].key, (u64)EMPTY_KEY, key);
      if (old == EMPTY_KEY) return true;
      if (old == key) return false;
    }
    h = (h + 1) & mask;
  }
  atomicOr(err, ERR_TABLE_FULL);
  return false;
}

// slot index of key, or ~0 if absent
__device__ __forceinline__ u64 table_find(const gm_slot* tab, u64 mask, u64 key) {
  u64 h = mix64(key) & mask;
  for (u64 probe = 0; probe <= mask; probe++) {
    u64 k = tab[h].key;
    if (k == key) return h;
    if (k == EMPTY_KEY) return ~0ull;
    h = (h + 1) & mask;
  }
  return ~0ull;
}

__device__ __forceinline__ u64 level_key(const u64* lv, u64 lcap, const LevelSeg& s, u64 i) {
  u64 nf = s.fe - s.fb;
  return i < nf ? lv[s.fb + i] : lv[lcap - 1 - (s.c2lo + (i - nf))];
}

// block-wide sum then one atomic per block
// per-block counts into this block's own slot (no atomics; launches on one
// stream run in order, so slot b has one writer at a time)
__device__ __forceinline__ void block_count(BlockCount* bc, u64 npos, u64 edges) {
  __shared__ u64 rn[16], re[16];
  for (int o = 32; o > 0; o >>= 1) {
    npos += __shfl_xor(npos, o);
    edges += __shfl_xor(edges, o);
  }
  const int w = threadIdx.x >> 6;
  if (__lane_id() == 0) {
    rn[w] = npos;
    re[w] = edges;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 sn = 0, se = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) {
      sn += rn[i];
      se += re[i];
    }
    if (sn | se) {
      bc[blockIdx.x].npos += sn;
      bc[blockIdx.x].edges += se;
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void block_add(u64* dst, u64 v) {
  __shared__ u64 red[16];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  int w = threadIdx.x >> 6;
  if (__lane_id() == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 s = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) s += red[i];
    if (s) atomicAdd(dst, s);
  }
  __syncthreads();
}

// Block-staged appends to up to two global stacks (Guideline 12).  Every
// new key used to cost one wave-aggregated atomic on ONE global cursor; a
// device-scope counter saturates near 90 adds/us, which bounded the hashed
// forward (toot 6x4: 324 ms on the widest level).  Keys now go to LDS with
// LDS atomics and a block reserves global space once per flush.  A key that
// finds its LDS queue full is appended straight to global memory (rare).
constexpr uint32_t kStageCap = 1024;  // keys per queue (2 queues: 16 KB, 8+ blocks per CU)
struct StageLDS {
  u64 key[2][kStageCap];
  uint32_t n[2];
  u64 base[2];
};

__device__ __forceinline__ void stage_init(StageLDS& s) {
  if (threadIdx.x == 0) s.n[0] = s.n[1] = 0;
  __syncthreads();
}

// queue q: true if staged, false if the caller must append directly
__device__ __forceinline__ bool stage_push(StageLDS& s, int q, u64 key) {
  const uint32_t j = atomicAdd(&s.n[q], 1u);
  if (j < kStageCap) {
    s.key[q][j] = key;
    return true;
  }
  return false;
}

// Block-uniform: true when a queue is at least 3/4 full.  Both barriers
// are needed so every thread reads the same counts before the next pushes.
__device__ __forceinline__ bool stage_should_flush(StageLDS& s) {
  __syncthreads();
  const bool f = s.n[0] >= kStageCap * 3 / 4 || s.n[1] >= kStageCap * 3 / 4;
  __syncthreads();
  return f;
}

// Reserve [base, base + n) on cursor q with one atomic per queue and copy
// the staged keys out with coalesced stores: store(q, global_index, key).
template <class Store>
__device__ __forceinline__ void stage_flush(StageLDS& s, u64* cur0, u64* cur1, Store store) {
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < 2; q++) {
      const uint32_t c = min(s.n[q], kStageCap);
      s.n[q] = c;
      s.base[q] = c ? atomicAdd(q ? cur1 : cur0, (u64)c) : 0;
    }
  }
  __syncthreads();
  for (int q = 0; q < 2; q++)
    for (uint32_t j = threadIdx.x; j < s.n[q]; j += blockDim.x) store(q, s.base[q] + j, s.key[q][j]);
  __syncthreads();
  if (threadIdx.x == 0) s.n[0] = s.n[1] = 0;
  __syncthreads();
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__global__ void k_seed(gm_slot* tab, u64 mask, u64* lv, DevState* st, u64 root) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    table_insert(tab, mask, root, &st->err);
    lv[0] = root;
    st->cursor_front = 1;
    st->cursor_back = 0;
    st->seg[0].fb = 0;
    st->seg[0].fe = 1;
    st->seg[0].c2lo = 0;
    st->seg[0].c2hi = 0;
    st->seg[1].c2lo = 0;
    st->seg[1].c2hi = 0;
  }
}

// append a new level-(L+1) key (q = 0, front stack) or level-(L+2) key
// (q = 1, back stack) at global stack index g
__device__ __forceinline__ void level_store(u64* lv, u64 lcap, int q, u64 g, u64 key) {
  if (g < lcap) lv[q ? lcap - 1 - g : g] = key;
}

// K1+K2: expand level L, insert children, append new ones to L+1 / L+2
// through the block's LDS stage (one global atomic per block flush).
template <int KIND>
__global__ __launch_bounds__(256) void k_expand(Desc d, gm_slot* tab, u64 mask, u64* lv, u64 lcap,
                                                DevState* st, int L) {
  __shared__ StageLDS stage;
  stage_init(stage);
  const LevelSeg s = st->seg[L];
  const u64 n = (s.fe - s.fb) + (s.c2hi - s.c2lo);
  const u64 stride = (u64)gridDim.x * blockDim.x;
  uint32_t err = 0;
  auto store = [&](int q, u64 g, u64 key) { level_store(lv, lcap, q, g, key); };
  for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += stride) {  // block-uniform
    const u64 i = base + threadIdx.x;
    if (i < n) {
      const u64 key = level_key(lv, lcap, s, i);
      if (Game<KIND>::prim(d, key) == UNDECIDED)  // lookup(): primitive, no children
        Game<KIND>::children(d, key, [&](u64 child, int step) {
          if (!table_insert(tab, mask, child, &st->err)) return;
          if (step != 1 && step != 2) {
            err |= ERR_BAD_STEP;
            return;
          }
          const int q = step - 1;
          if (!stage_push(stage, q, child))
            store(q, atomicAdd(q ? &st->cursor_back : &st->cursor_front, 1ull), child);
        });
    }
    if (stage_should_flush(stage)) stage_flush(stage, &st->cursor_front, &st->cursor_back, store);
  }
  stage_flush(stage, &st->cursor_front, &st->cursor_back, store);
  if (err) atomicOr(&st->err, err);
}

// level bookkeeping after expanding level L (one thread)
__global__ void k_finalize(DevState* st, int L, u64 lcap) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    LevelSeg& nx = st->seg[L + 1];
    nx.fb = st->seg[L].fe;
    nx.fe = st->cursor_front;
    LevelSeg& nn = st->seg[L + 2];
    nn.c2lo = nx.c2hi;
    nn.c2hi = st->cursor_back;
    if (st->cursor_front + st->cursor_back > lcap) st->err |= ERR_LEVELS_FULL;
    u64 w = (nx.fe - nx.fb) + (nx.c2hi - nx.c2lo);
    if (w > st->max_width) st->max_width = w;
  }
}

// K3: resolve level L from its children's words
template <int KIND>
__global__ __launch_bounds__(256) void k_resolve(Desc d, gm_slot* tab, u64 mask, const u64* lv, u64 lcap,
                                                 DevState* st, int L) {
  const LevelSeg s = st->seg[L];
  const u64 n = (s.fe - s.fb) + (s.c2hi - s.c2lo);
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u64 edges = 0, prims = 0;
  uint32_t err = 0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u64 key = level_key(lv, lcap, s, i);
    int p = Game<KIND>::prim(d, key);
    uint32_t word;
    if (p != UNDECIDED) {
      word = make_word(p, 0);  // process.py:120-123: primitive, remoteness 0
      prims++;
    } else {
      bool any_loss = false, any_tie = false, any_draw = false;
      uint32_t min_loss = 0xFFFFFFFFu, max_all = 0;
      int nch = Game<KIND>::children(d, key, [&](u64 c, int) {
        u64 h = table_find(tab, mask, c);
        if (h == ~0ull) { err |= ERR_CHILD_MISSING; return; }
        uint32_t w = tab[h].word;
        if (w == NO_WORD) { err |= ERR_CHILD_UNRESOLVED; return; }
        uint32_t v = w & 3u, r = w >> 2;
        if (v == LOSS) { any_loss = true; min_loss = min(min_loss, r); }
        any_tie |= (v == TIE);
        any_draw |= (v == DRAW);
        max_all = max(max_all, r);
      });
      if (nch == 0) err |= ERR_NO_MOVES;
      edges += (u64)nch;
      // reference-canonical _res_red / _remote_red
      if (any_loss) word = make_word(WIN, min_loss + 1);
      else word = make_word(any_tie ? TIE : any_draw ? DRAW : LOSS, max_all + 1);
    }
    u64 h = table_find(tab, mask, key);
    if (h == ~0ull) err |= ERR_SELF_MISSING;
    else tab[h].word = word;
  }
  if (err) atomicOr(&st->err, err);
  block_add(&st->edges, edges);
  block_add(&st->prims, prims);
}

// word of `key` in the hash table (NO_WORD if absent): HashedWords (gm_table.h)
__device__ __forceinline__ uint32_t hashed_word(const Desc& d, const gm_slot* tab, u64 mask, u64 key) {
  u64 h = table_find(tab, mask, any_canon(d, key));  // symmetry hooks: the orbit's representative
  return h == ~0ull ? NO_WORD : tab[h].word;
}

__global__ void k_root_word(const gm_slot* tab, u64 mask, u64 root, DevState* st) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u64 h = table_find(tab, mask, root);
    st->root_word = h == ~0ull ? NO_WORD : tab[h].word;
  }
}


#include "gm_dense.h"
#include "gm_keyed_shard.h"

// K4 owner kernel: md5(str(pos)) % P per key (GameState.get_hash,
// src/game_state.py:22-30), the register-resident form where it applies
__global__ void k_owner(Desc d, const u64* keys, u64 n, uint32_t P, uint32_t* owners) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
    owners[i] = owner_dev(d, keys[i], P);
}
#include "gm_bucketed.h"

// ---------------------------------------------------------------------------
// solver object
// ---------------------------------------------------------------------------
// Dense kernel families, fixed when the solver is created (dense_choose,
// from the descriptor, the shard geometry and the GM_F_* flags of
// gm_buffers): nothing later -- no environment variable, no flag change --
// can hand a table a kernel of another word width.  The codes are reported
// in gm_result.kernels (resolve | pull << 16).
// RANKED layout geometry (gm_ranked.h): toot-and-otto positions at computed
// indices
constexpr int kRankMaxCols = 8;
struct RankGeom {
  uint32_t C, H, R, A;     // columns, rows, height radix H + 1, cells
  uint32_t T;              // levels (pieces 0 .. A)
  uint32_t stride[kRankMaxCols];  // hvcode stride of column x: R^x
  u64 nslots;
  uint8_t* words;          // [nslots]
  uint32_t* reach;         // [nslots / 32] reached
  uint32_t* expd;          // [nslots / 32] reached and not primitive
  const u64* base;         // [R^C] hvcode -> first slot of its block
  const uint32_t* lvhv;    // hvcodes level by level
  const uint32_t* lvph;    // the same, heights packed 4 bits per column
  const uint32_t* lvch;    // per block entry, kRankMaxCols u32: child block x's first slot - its level's
                           // first slot (0xFFFFFFFF: column x full)
  const uint32_t* lvpa;    // per block entry, kRankMaxCols u32: parent block x (column x's top piece
                           // removed)'s first slot - its level's first slot (0xFFFFFFFF: column x empty)
  uint8_t* bstat;          // [nslots / 8] per board (stacks): primitive value or UNDECIDED
  u64* pbits;              // [nslots / 512] per board: primitive
  u64 le[7];               // bits j < 64 with popcount(j) <= c
};
// RANKED layout geometry of connect four (gm_ranked_connect.h): a height
// vector's block is its 2^L stack patterns (bit = 1: an X piece), no hands.
// Blocks are named by their ORDINAL inside their level (all blocks of a level
// have 2^L slots): block j of level L starts at slot lvstart[L] + (j << L),
// a 64-bit sum -- levels of 6x5 and 5x6 pass 2^32 slots.
struct C4Geom {
  uint32_t C, H, R, A;     // columns, rows, height radix H + 1, cells
  uint32_t T;              // levels (pieces 0 .. A)
  uint32_t stride[kRankMaxCols];  // hvcode stride of column x: R^x
  uint32_t spread;         // C > H: a column's stack reaches its cells by one multiply (mul, msk)
  uint32_t mul, msk;       // sum of 2^((C-1) y), sum of 2^(C y), y < H
  u64 nslots;
  uint8_t* words;          // [nslots] the board pass' primitive value / UNDECIDED, then the solved word
  uint32_t* reach;         // [nslots / 32] reached
  uint32_t* expd;          // [nslots / 32] reached and not primitive
  u64* pbits;              // [nslots / 64] primitive (or no position: unbalanced colours)
  const u64* lvstart;      // [T + 1] per level: first slot (512-aligned)
  const uint32_t* lvoff;   // [T + 1] per level: first entry of its block list
  const uint32_t* ord;     // [R^C] hvcode -> ordinal of its block in its level
  const uint32_t* lvph;    // per block entry: heights packed 4 bits per column
  const uint32_t* lvch;    // per block entry, kRankMaxCols u32: child block x's ordinal in level L + 1
                           // (0xFFFFFFFF: column x full)
  const uint32_t* lvpa;    // per block entry, kRankMaxCols u32: parent block x's ordinal in level L - 1
                           // (0xFFFFFFFF: column x empty)
  u64 eq[7];               // bits j < 64 with popcount(j) == c
};

enum DenseResolveKind : uint32_t {
  RK_NONE = 0,
  RK_OCT_LIST = 1,   // k_dense_resolve8p: world 1, 16-bit table, live-group lists
  RK_OCT_COLS = 2,   // k_dense_resolve8c: shards, 16-bit table, column jobs
  RK_QUAD_LIST = 3,  // k_dense_resolve4p: world 1, 32-bit table, live-group lists
  RK_QUAD_COLS = 4,  // k_dense_resolve4c: shards, 32-bit table, column jobs
  RK_QUAD_BAND = 5,  // k_dense_resolve4: 32-bit band sweeps (no list)
  RK_SCALAR = 6,     // k_dense_resolve: one prefix per lane (any bases; GM_F_RESOLVE_SCALAR)
  RK_HEX_LIST = 7,   // k_dense_resolve16p: world 1, 8-bit table, live-group lists
  RK_PLANE = 8,      // k_plane_resolve: PLANES layout (gm_plane.h), one plane per half-wave
  RK_PLANE_X2 = 9,   // k_plane_resolve_x2: two planes per half-wave, packed 16-bit lanes
  RK_RANKED = 10,    // k_rk_backward: RANKED layout (gm_ranked.h)
  RK_PLANE_FLOW = 11,  // k_plane_flow: the one-launch PLANES backward (gm_plane.h)
  RK_RANKED_CONNECT = 12,  // k_c4_backward: RANKED layout of connect four (gm_ranked_connect.h)
};
enum DensePullKind : uint32_t { PK_NONE = 0, PK_WORDS = 1, PK_LANE = 2, PK_PLANE = 3 };
struct TbGeom;  // an opened tablebase file's sections (gm_table_file.h)
struct TkGeom;

struct gm_solver {
  Desc d;
  uint32_t mode;
  uint32_t* words;  // DENSE table: levels * Wl words ...
  u64* bits;        // ... followed by the reach bitmap (levels * Wbl bits)
  DenseView view;   // owned prefix range + local addressing
  u64 nslots;       // DENSE: levels * Wl
  // dense sharding over the top prefix digit
  int rank, world;
  u64 nblocks;  // blocks of the top digit over all ranks (view.B values each)
  ncclComm_t comm;  // RCCL communicator (world > 1), or null
  u64* errg = nullptr;  // RCCL: every rank's error mask, all-gathered (world u64, device)
  gm_xfer_fn xfer = nullptr;  // host-staged transport (gm_solver_set_transport), replaces comm
  void* xfer_ctx = nullptr;
  bool halo_ok = false;       // the exchange plan was checked against the other ranks'
  std::vector<uint8_t> hstage;  // host staging of the transport
  gm_slot* tab;
  u64 mask;
  u64* lv;
  u64 lcap;
  DevState* st;
  const u64* masks;  // dense pow2 mask tables in scratch (k_dense_pull_words)
  // sharded dense solves: halo exchanges run on their own stream, ordered
  // against the compute stream by events (created on first use)
  hipStream_t cstream = nullptr;
  std::vector<hipEvent_t> pev;
  // packed word halos (HaloGeom): device offset table, buffers, host totals
  HaloGeom hg;
  HaloTabs ht{};
  bool halo16 = false;  // words travel as 16 bits (k_halo_cols)
  bool w16 = false;     // this solve's table holds 16-bit order-form words (k_dense_resolve8p / 8c)
  bool w8 = false;      // 8-bit order-form words (k_dense_resolve16p)
  uint32_t wbits() const { return w8 ? 8u : w16 ? 16u : 32u; }
  uint32_t plan_bits = 32;  // the table's word width as planned (dense_plan_bits)
  BlockCount* bcount = nullptr;  // per-block counts in scratch (block_count)
  uint32_t* halo_send = nullptr;
  uint32_t* halo_recv = nullptr;
  std::vector<uint32_t> halo_tot;
  // active-group lists (GroupGeom): device list, per-level offsets and
  // per-level XCD shares (host)
  const uint32_t* glist = nullptr;
  std::vector<u64> goff;
  std::vector<uint32_t> gxcd;  // [L * 9 + x]: share x of level L starts at entry gxcd (relative to goff[L])
  // column permutation (ColGeom): device perm, host cstart
  const uint32_t* colperm = nullptr;
  ColGeom cg;
  std::vector<uint32_t> cstart;
  hipStream_t stream;
  bool own_stream;
  uint32_t flags;
  int grid;
  uint32_t step_first = 0, step_stop = 0;  // gm_solver_set_steps (one solve)
  uint32_t rk = RK_NONE, pk = PK_NONE;      // dense kernel families (dense_choose)
  bool launch_err = false;                  // a launch found no kernel of the table's word width
  bool solved = false;  // the buffers hold a finished full solve (gm_solver_moves / _line / _audit need one)
  // whole-solve HIP graphs of a one-table dense solve (run_dense): the
  // forward and the backward launches, captured on the first full solve
  hipGraphExec_t gfwd = nullptr, gbwd = nullptr;
  // one-table PLANES: the counts of a solve in pinned host memory, the
  // solve's timing events, and the ring of queued solves
  // (gm_solver_solve_async / gm_solver_collect)
  u64* phost = nullptr;
  hipEvent_t pse[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // run_planes' events (as PlaneSlot::ev)
  PlaneSlot pring[kPlaneRing];
  u64 pq_next = 0, pq_done = 0;  // tickets issued / collected
  // BUCKETED (gm_bucketed.h): level store, words, in-edges, partition scratch
  u64* bkK = nullptr;
  uint32_t* bkW = nullptr;
  uint32_t* REp = nullptr;
  uint16_t* REc = nullptr;  // child index inside its bucket (< kBkMaxUnique)
  u64* S1k = nullptr;
  uint32_t* S1p = nullptr;
  u64* S2k = nullptr;
  uint8_t* S1f = nullptr;  // per staged child: the byte under mix64's top byte (fine bucket bits)
  u64 *XSk = nullptr, *XRk = nullptr;  // md5-sharded bucketed levels: exchange buffers
  uint32_t *XSr = nullptr, *XRr = nullptr;
  std::vector<std::vector<u64>> bks_sc, bks_rc;  // per forward level: records sent to / received from each rank
  uint32_t* REpl = nullptr;  // md5 shards, local-dedup form: in-edges of the rank's own parents' children
  uint16_t* REcl = nullptr;
  struct BksLocal {
    u64 rb = 0, ein = 0, nu = 0;  // local in-edges [rb, rb + ein), unique local children
    uint32_t nbits = 0, cst_off = 0;
    bool used = false;  // this level's children went out in the local-dedup form
  };
  std::vector<BksLocal> bksl;  // per parent level
  u64* xdev = nullptr;  // RCCL all-gather staging of the sharded bucketed loop
  size_t xdev_n = 0;
  u64 Pcap = 0, Ecap = 0, Emax = 0;
  BkLevel* bkL = nullptr;  // device level table (scratch)
  uint32_t *pbase = nullptr, *bh = nullptr, *ph = nullptr, *boff = nullptr, *tot = nullptr, *cbase = nullptr;
  uint32_t *bkcur = nullptr, *bkah = nullptr, *ucnt = nullptr, *meta = nullptr;
  uint32_t* bkgc = nullptr;  // [256 partition cursors | 256 parent-range totals | overflow flag]
  u64* bktotal = nullptr;
  u64 meta_cap = 0;
  std::vector<BkLevel> lvh;  // host copy of the level table
  // PLANES (gm_plane.h, gm_plane_run.h)
  PlaneGeom pg{};
  uint32_t pwb = 1;     // word bytes
  uint32_t pform = 1;   // word form: 1 8-bit, 2 16-bit, 3 relative 8-bit (gm_plane.h)
  // DevState::word_bits of a planes solve in progress (a resume checks it):
  // the word width, 0x100 set for the relative forms
  uint32_t pmark() const { return 8u * pwb | (pform == 3 ? 0x100u : 0u); }
  uint32_t pS = 0;      // last plane level
  void* ptab = nullptr;  // words
  uint32_t* pbits = nullptr;  // reach map, 32 bits per plane row
  void* precv = nullptr;  // shard halo planes received / sent (all levels)
  void* psend = nullptr;
  u64 pnrecv = 0, pnsend = 0;
  const uint4* pzero = nullptr;  // 4 KB of zeros (absent neighbours)
  const void* plist = nullptr;   // level lists (uint32 planes, or PlaneEntry for shards)
  std::vector<u64> ploff;        // per level: first list entry
  std::vector<u64> pbnd;         // shards, per level: first entry that reads a halo plane (they come last)
  std::vector<u64> prcv_off, psnd_off;  // shards, per level: first halo plane received / sent
  // the one-launch backward (k_plane_flow; one-table 8-bit absolute solves):
  // visit lists, counters and per-plane flags in the scratch buffer
  PlaneFlow pflow{};
  bool pflow_ok = false;
  bool pflow_last = false;  // the last solve's backward was k_plane_flow
  uint32_t pflow_grid = 0;
  // staged PLANES shards (run_planes_staged): ploff / prcv_off / psnd_off are
  // per key / per row; k = key skew, K keys, rows 0..smax
  uint32_t pstage_k = 0, pkeys = 0, prows = 0;
  ncclComm_t comm2 = nullptr;        // second communicator (ncclCommSplit): the other halo direction
  // the group's abort flag (solve_multi): once set, its communicators are
  // being aborted and this shard issues no further RCCL call
  std::atomic<int>* gabort = nullptr;
  int defer_rc = 0;                  // a deferred failure of this shard's last solve (0: none)
  std::string defer_msg;
  hipStream_t cstream2 = nullptr;    // receive stream of the staged exchange
  // RANKED (gm_ranked.h)
  RankGeom rg{};
  std::vector<uint32_t> rlvoff;        // per level: first entry of its block list
  std::vector<u64> rlvstart, rlvitems;  // per level: first slot, slots
  u64* rlv_dev = nullptr;              // device: rlvstart then rlvoff (RankEnum's lvt)
  // RANKED, connect four (gm_ranked_connect.h): rlvoff / rlvstart / rlvitems as
  // above; the index tables live in an allocation of the solver's own
  C4Geom kg{};
  void* c4_dev = nullptr;
  u64* cen_dev = nullptr;              // device: gm_solver_census' counts, maxima and witnesses (gm_census.h)
  // gm_solver_export (gm_export.h): block offsets and totals of a call (device,
  // grown on demand); for toot tables of the keyed layouts the level tables
  // and packed heights of the RANKED index map (xg.lvph, the lvt halves)
  u64* exp_dev = nullptr;
  size_t exp_words = 0;
  u64* xgeo_dev = nullptr;
  RankGeom xg{};
  // md5 shards of the RANKED layout (gm_ranked_shard.h), inside the table
  // buffer: every slot's owner, the level pack / receive buffers, per-level
  // tile counts, their offsets and totals (device; the totals also on the host)
  uint4* rko_own = nullptr;  // owner bit planes, 16 B per 32 slots
  uint8_t *rko_pk = nullptr, *rko_rb = nullptr;
  uint32_t *rko_cnt = nullptr, *rko_toff = nullptr;
  u64* rko_tot = nullptr;
  std::vector<u64> rko_tile0, rko_tot_h;
  // GM_MODE_FILE (gm_table_file.h): the sections of the opened image, one of
  // the two by the file's format (1 gmtb, 2 gmtk), and its word bytes
  TbGeom* tb = nullptr;
  TkGeom* tk = nullptr;
  uint32_t tf_format = 0, tf_wb = 0;
};

static const int kBlock = 256;

static int launch_grid() {
  static int g = 0;
  if (!g) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
    }
    g = cus * 8;  // Guideline 11: 8 blocks/CU, grid-stride the rest
  }
  return g;
}

// one HASHED level: the kernel of the descriptor's kind, symmetric where it
// asks for orbit representatives (gm_sym.h)
static void do_expand(gm_solver* s, int L) {
  kind_dispatch_sym<GenericKinds>(s->d, s->d.kind, [&](auto kind_) {
    hipLaunchKernelGGL(k_expand<decltype(kind_)::value>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, s->tab, s->mask,
                       s->lv, s->lcap, s->st, L);
  });
}
static void do_resolve(gm_solver* s, int L) {
  kind_dispatch_sym<GenericKinds>(s->d, s->d.kind, [&](auto kind_) {
    hipLaunchKernelGGL(k_resolve<decltype(kind_)::value>, dim3(s->grid), dim3(kBlock), 0, s->stream, s->d, s->tab,
                       s->mask, s->lv, s->lcap, s->st, L);
  });
}

static std::string err_text(uint32_t e) {
  std::string s;
  if (e & ERR_TABLE_FULL) s += " table-full";
  if (e & ERR_LEVELS_FULL) s += " level-store-full";
  if (e & ERR_BAD_STEP) s += " bad-level-step";
  if (e & ERR_CHILD_MISSING) s += " child-missing";
  if (e & ERR_CHILD_UNRESOLVED) s += " child-unresolved";
  if (e & ERR_NO_MOVES) s += " non-primitive-without-moves";
  if (e & ERR_SELF_MISSING) s += " self-missing";
  if (e & ERR_BUCKET_FULL) s += " hash-bucket-over-capacity";
  if (e & ERR_EDGE_COUNT) s += " edge-count-mismatch";
  if (e & ERR_SHARD_FAILED) s += " shard-failed";
  if (e & ERR_PLANE_STALL) s += " plane-flow-stalled";
  return s;
}

// HASHED solve of one keyed table (the pipeline of the file header)
static int run_hashed(gm_solver* s, gm_result* out) {
  const int T = s->d.max_levels;
  // steps [first, stop) of the 2T (gm_solver_set_steps); forward level L is
  // step L (level T-1 expands nothing), backward level L is step 2T-1-L
  const int first = (int)s->step_first, stop = s->step_stop ? (int)s->step_stop : 2 * T;
  s->step_first = s->step_stop = 0;
  const bool timing = (s->flags & GM_F_KERNEL_TIMING) && first == 0 && stop == 2 * T;
  SolveEvents ev;  // kx / kr: per-launch start/stop pairs
  if (ev.begin(timing ? (size_t)T : 0)) return GM_EHIP;
  auto t0 = std::chrono::steady_clock::now();
  HIPCHK(hipEventRecord(ev.e0, s->stream));
  if (first == 0) {
    // fresh table: keys EMPTY, words NO_WORD
    HIPCHK(hipMemsetAsync(s->tab, 0xFF, (s->mask + 1) * sizeof(gm_slot), s->stream));
    HIPCHK(hipMemsetAsync(s->st, 0, devstate_bytes(T), s->stream));
    hipLaunchKernelGGL(k_seed, dim3(1), dim3(64), 0, s->stream, s->tab, s->mask, s->lv, s->st, s->d.root);
  }
  for (int L = std::max(first, 0); L + 1 < T && L < stop; L++) {
    if (timing) HIPCHK(hipEventRecord(ev.kx[2 * L], s->stream));
    do_expand(s, L);
    if (timing) HIPCHK(hipEventRecord(ev.kx[2 * L + 1], s->stream));
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s->stream, s->st, L, s->lcap);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e1, s->stream));
  for (int L = T - 1; L >= 0; L--) {
    const int k = 2 * T - 1 - L;
    if (k < first) continue;
    if (k >= stop) break;
    if (timing) HIPCHK(hipEventRecord(ev.kr[2 * L], s->stream));
    do_resolve(s, L);
    if (timing) HIPCHK(hipEventRecord(ev.kr[2 * L + 1], s->stream));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e2, s->stream));
  if (stop < 2 * T) {  // stopped early: the state stays on the device for a resume
    HIPCHK(hipStreamSynchronize(s->stream));
    out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GM_PARTIAL;
  }
  hipLaunchKernelGGL(k_root_word, dim3(1), dim3(64), 0, s->stream, s->tab, s->mask, s->d.root, s->st);
  HIPCHK(hipGetLastError());
  std::vector<unsigned char> host(devstate_bytes(T));
  HIPCHK(hipMemcpyAsync(host.data(), s->st, host.size(), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  auto t1 = std::chrono::steady_clock::now();
  const DevState* hs = (const DevState*)host.data();
  const uint32_t word = hs->root_word;
  float f = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&f, ev.e0, ev.e1));
  HIPCHK(hipEventElapsedTime(&b, ev.e1, ev.e2));
  out->ms_forward = f;
  out->ms_backward = b;
  out->ms_total = std::chrono::duration<double, std::milli>(t1 - t0).count();
  if (timing) {
    if (SolveEvents::pairs_ms(ev.kx, T - 1, &out->ms_expand_kernels)) return GM_EHIP;
    if (SolveEvents::pairs_ms(ev.kr, T, &out->ms_resolve_kernels)) return GM_EHIP;
    out->n_expand_launches = (uint64_t)(T - 1);
    out->n_resolve_launches = (uint64_t)T;
  }
  out->positions = hs->cursor_front + hs->cursor_back;
  out->edges = hs->edges;
  out->primitives = hs->prims;
  out->max_level_width = (uint32_t)std::max<u64>(hs->max_width, 1);
  uint32_t lv = 0;
  for (int L = 0; L < T; L++) {
    const LevelSeg& g = hs->seg[L];
    if ((g.fe - g.fb) + (g.c2hi - g.c2lo) > 0) lv++;
  }
  out->levels = lv;
  out->root_word = word;
  if (hs->err) {
    bool full = hs->err & (ERR_TABLE_FULL | ERR_LEVELS_FULL);
    return fail(full ? GM_EFULL : GM_ECORRUPT, "solve failed:%s", err_text(hs->err).c_str());
  }
  if (word == NO_WORD) return fail(GM_ECORRUPT, "root unresolved");
  out->root_value = (int32_t)(word & 3u);
  out->root_remoteness = word >> 2;
  return 0;
}


// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

const char* gm_last_error(void) { return g_err.c_str(); }
const char* gm_version(void) { return "gamesmanmpi_amd 0.1 (gfx950)"; }

int gm_abi_sizes(uint32_t out[3]) {
  if (!out) return fail(GM_EINVAL, "null argument");
  out[0] = (uint32_t)sizeof(gm_plan_t);
  out[1] = (uint32_t)sizeof(gm_buffers);
  out[2] = (uint32_t)sizeof(gm_result);
  return 0;
}

// (gm_game_lookup, gm_game_info, gm_root: gm_registry.h)
int gm_encode(int game, const uint8_t* canon, size_t n, uint64_t* key) {
  const Desc* d = get_game(game);
  if (!d || !canon || !key) return fail(GM_EINVAL, "bad argument");
  char why[96];
  if (key_from_canon(*d, canon, n, key, why)) return fail(GM_EINVAL, "%s", why);
  return 0;
}

int gm_decode(int game, uint64_t key, uint8_t* canon, size_t cap, size_t* n) {
  const Desc* d = get_game(game);
  if (!d || !canon || !n) return fail(GM_EINVAL, "bad argument");
  uint8_t tmp[64];
  int m = canon_from_key(*d, key, tmp);
  if ((size_t)m > cap) return fail(GM_EINVAL, "buffer too small");
  memcpy(canon, tmp, (size_t)m);
  *n = (size_t)m;
  return 0;
}

int gm_encode_batch(int game, const uint8_t* canon, size_t stride, const uint8_t* lens, size_t n,
                    uint64_t* keys) {
  for (size_t i = 0; i < n; i++) {
    int rc = gm_encode(game, canon + i * stride, lens[i], &keys[i]);
    if (rc) return rc;
  }
  return 0;
}

int gm_decode_batch(int game, const uint64_t* keys, size_t n, uint8_t* canon, size_t stride, uint8_t* lens) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !canon || !lens))) return fail(GM_EINVAL, "bad argument");
  for (size_t i = 0; i < n; i++) {
    uint8_t tmp[64];
    int m = canon_from_key(*d, keys[i], tmp);
    if ((size_t)m > stride) return fail(GM_EINVAL, "stride too small");
    memset(canon + i * stride, 0, stride);
    memcpy(canon + i * stride, tmp, (size_t)m);
    lens[i] = (uint8_t)m;
  }
  return 0;
}

int gm_str_utf8(int game, uint64_t key, uint8_t* out, size_t cap, size_t* n) {
  const Desc* d = get_game(game);
  if (!d || !out || !n) return fail(GM_EINVAL, "bad argument");
  uint8_t tmp[64];
  int m = str_utf8_from_key(*d, key, tmp);
  if ((size_t)m > cap) return fail(GM_EINVAL, "buffer too small");
  memcpy(out, tmp, (size_t)m);
  *n = (size_t)m;
  return 0;
}

int gm_host_expand(int game, const uint64_t* keys, size_t n, uint64_t* children, uint8_t* nchild, uint8_t* prim) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !children || !nchild || !prim))) return fail(GM_EINVAL, "bad argument");
  for (size_t i = 0; i < n; i++) {
    prim[i] = (uint8_t)any_prim(*d, keys[i]);
    int c = 0;
    if (prim[i] == UNDECIDED)
      any_children(*d, keys[i], [&](uint64_t ck, int) {
        if (c < GM_MAXCHILD) children[i * GM_MAXCHILD + c] = ck;
        c++;
      });
    if (c > GM_MAXCHILD) return fail(GM_ECORRUPT, "more than %d children", GM_MAXCHILD);
    nchild[i] = (uint8_t)c;
  }
  return 0;
}

int gm_host_level(int game, const uint64_t* keys, size_t n, int32_t* levels) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !levels))) return fail(GM_EINVAL, "bad argument");
  for (size_t i = 0; i < n; i++) levels[i] = any_level(*d, keys[i]);
  return 0;
}

int gm_symmetry_count(int game, uint32_t* count) {
  const Desc* d = get_game(game);
  if (!d || !count) return fail(GM_EINVAL, "bad argument");
  *count = d->bsym ? (uint32_t)sym_board_maps(*d) : d->sym ? 1u : 0u;
  return 0;
}

int gm_symmetry(int game, int which, const uint64_t* keys, size_t n, uint64_t* out) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !out))) return fail(GM_EINVAL, "bad argument");
  if (which == -1) {
    for (size_t i = 0; i < n; i++) out[i] = any_canon(*d, keys[i]);
    return 0;
  }
  if (d->bsym) {
    if (which < 0 || which >= sym_board_maps(*d))
      return fail(GM_EINVAL, "no board map %d for this game (%d maps)", which, sym_board_maps(*d));
    for (size_t i = 0; i < n; i++) out[i] = sym_board_map(*d, keys[i], which);
    return 0;
  }
  if (which != 0 || d->kind != K_OTHELLO) return fail(GM_EINVAL, "no symmetry function %d for this game", which);
  for (size_t i = 0; i < n; i++) out[i] = oth_flip(*d, keys[i]);
  return 0;
}

int gm_owner_host(int game, const uint64_t* keys, size_t n, int world_size, uint32_t* owners) {
  const Desc* d = get_game(game);
  if (!d || world_size < 1 || (n && (!keys || !owners))) return fail(GM_EINVAL, "bad argument");
  for (size_t i = 0; i < n; i++) {
    uint8_t s[64], dig[16];
    int len = str_utf8_from_key(*d, keys[i], s);
    md5_block(s, len, dig);
    owners[i] = md5_mod(dig, (uint32_t)world_size);
  }
  return 0;
}

int gm_shard_info(int game, int rank, int world, uint64_t out[8]) {
  const Desc* d = get_game(game);
  if (!d || !out) return fail(GM_EINVAL, "bad argument");
  if (!d->dense_ok) return fail(GM_EINVAL, "game has no dense layout");
  DenseGeom g;
  int rc = dense_geom(d, rank, world, &g);
  if (rc) return rc;
  const uint64_t v[8] = {g.v.B, g.nblocks, g.nb, (uint64_t)rank, g.v.Z, g.v.E, g.v.Wl, (uint64_t)world};
  memcpy(out, v, sizeof v);
  return 0;
}

// the per-block counts summed into the table's totals and the solve's
// reduction words (one block of 1024 threads; also the tail of the PLANES
// finish kernel, k_plane_finish)
__device__ __forceinline__ void fill_red_body(DevState* st, const BlockCount* bc) {
  __shared__ u64 rn[16], re[16];
  u64 sn = 0, se = 0;
  for (int i = (int)threadIdx.x; i < kCountSlots; i += (int)blockDim.x) {
    sn += bc[i].npos;
    se += bc[i].edges;
  }
  for (int o = 32; o > 0; o >>= 1) {
    sn += __shfl_xor(sn, o);
    se += __shfl_xor(se, o);
  }
  if (__lane_id() == 0) {
    rn[threadIdx.x >> 6] = sn;
    re[threadIdx.x >> 6] = se;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sn = se = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) {
      sn += rn[w];
      se += re[w];
    }
    st->cursor_front += sn;  // this table's totals (gm_solver_positions reads them)
    st->edges += se;
    st->red[0] = st->cursor_front;
    st->red[1] = st->edges;
    st->red[2] = st->prims;
    st->red[3] = st->root_word == NO_WORD ? 0 : (u64)st->root_word + 1;
    st->red[4] = st->err;
  }
}
__global__ __launch_bounds__(1024) void k_fill_red(DevState* st, const BlockCount* bc) { fill_red_body(st, bc); }

// the layouts' host paths (and the kernels that need DevState / gm_solver)
#include "gm_xchg.h"
#include "gm_dense_run.h"
#include "gm_plane_run.h"
#include "gm_ranked.h"
#include "gm_ranked_shard.h"
#include "gm_ranked_connect.h"
#include "gm_bucketed_run.h"
#include "gm_bucketed_shard.h"
#include "gm_table_file.h"

int gm_rk_shard_stats(gm_solver* s, uint64_t out[2]) {
  if (!s || !out) return fail(GM_EINVAL, "bad argument");
  if (s->mode != GM_MODE_RANKED || s->world < 2 || !s->rko_own) return fail(GM_EINVAL, "not a ranked md5 shard");
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipMemcpy(&out[0], &s->st->ks_cursor, sizeof(u64), hipMemcpyDeviceToHost));
  out[1] = 0;
  for (size_t L = 0; L < s->rko_tot_h.size() / (size_t)s->world; L++) out[1] += s->rko_tot_h[L * s->world + s->rank];
  return 0;
}

int gm_plane_halo_plan(int game, int rank, int world, uint32_t flags, uint64_t* out, uint32_t levels) {
  const Desc* d = get_game(game);
  if (!d || !out || world < 2 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad argument");
  if (!plane_ok(d, world)) return fail(GM_EINVAL, "game has no planes layout");
  PlaneShape ps;
  int rc = plane_shape(d, rank, world, flags, &ps);
  if (rc) return rc;
  const uint32_t steps = ps.stage_k ? ps.nrows : ps.S + 1;
  if (levels < steps) return fail(GM_EINVAL, "out holds %u steps, the plan has %u", levels, steps);
  memset(out, 0, (size_t)levels * world * 2 * sizeof(uint64_t));
  std::unique_ptr<gm_solver> s(new gm_solver());
  s->world = world;
  s->rank = rank;
  std::vector<uint8_t> lb;
  rc = plane_lists(s.get(), ps, lb);
  if (rc) return rc;
  if (ps.stage_k) {  // staged: step = halo row, to rank + 1 / from rank - 1
    for (uint32_t r = 0; r < ps.nrows; r++) {
      if (rank + 1 < world) out[((size_t)r * world + rank + 1) * 2] = s->psnd_off[r + 1] - s->psnd_off[r];
      if (rank > 0) out[((size_t)r * world + rank - 1) * 2 + 1] = s->prcv_off[r + 1] - s->prcv_off[r];
    }
    return 0;
  }
  for (uint32_t l = 0; l <= ps.S; l++)
    for (int p = 0; p < world; p++) {
      u64 n;
      plane_seg(s->psnd_off, l, world, p, &n);
      out[((size_t)l * world + p) * 2] = n;
      plane_seg(s->prcv_off, l, world, p, &n);
      out[((size_t)l * world + p) * 2 + 1] = n;
    }
  return 0;
}

int gm_plan_shard(int game, int rank, int world, uint32_t flags, uint64_t max_table_bytes, gm_plan_t* out) {
  const Desc* d = get_game(game);
  if (!d || !out) return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  out->max_levels = (uint32_t)d->max_levels;
  out->scratch_bytes = scratch_bytes_for(d->max_levels);
  if (!d->dense_ok || (flags & GM_F_FORCE_HASHED))
    return fail(GM_EINVAL, "only DENSE layouts shard by prefix blocks; keyed tables shard by md5 owner");
  if (plane_wanted(d, flags, world)) {
    bool fits = false;
    int rc = plan_planes(d, rank, world, flags, max_table_bytes, out, &fits);
    if (rc) return rc;
    if (!fits) return fail(GM_EFULL, "planes shard needs %llu bytes", (unsigned long long)out->table_bytes);
    return 0;
  }
  DenseGeom g;
  int grc = dense_geom(d, rank, world, &g);
  if (grc) return grc;
  out->scratch_bytes += halo_bytes(halo_geom(d, world, g.nb)) + col_bytes(d);
  bool fits = false;
  int rc = plan_dense(d, rank, world, flags, max_table_bytes, out, &fits);
  if (rc) return rc;
  if (!fits) return fail(GM_EFULL, "dense shard needs %llu bytes", (unsigned long long)out->table_bytes);
  return 0;
}

int gm_plan(int game, uint64_t positions, uint32_t flags, uint64_t max_table_bytes, gm_plan_t* out) {
  const Desc* d = get_game(game);
  if (!d || !out) return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  out->max_levels = (uint32_t)d->max_levels;
  out->scratch_bytes = scratch_bytes_for(d->max_levels);
  if (d->dense_ok && plane_wanted(d, flags, 1)) {
    bool fits = false;
    int rc = plan_planes(d, 0, 1, flags, max_table_bytes, out, &fits);
    if (rc) return rc;
    if (fits) return 0;
    memset(out, 0, sizeof *out);
    out->max_levels = (uint32_t)d->max_levels;
    out->scratch_bytes = scratch_bytes_for(d->max_levels);
  }
  if (d->dense_ok && !(flags & GM_F_FORCE_HASHED)) {
    bool fits = false;
    int rc = plan_dense(d, 0, 1, flags, max_table_bytes, out, &fits);
    if (rc) return rc;
    out->scratch_bytes += col_bytes(d) + group_bytes(d, 1);
    if (fits) return 0;
    memset(out, 0, sizeof *out);
    out->max_levels = (uint32_t)d->max_levels;
    out->scratch_bytes = scratch_bytes_for(d->max_levels);
  }
  if ((flags & GM_F_RANKED) && d->kind == K_CONNECT) {  // on request: connect four at computed indices
    if (const char* why = c4_rank_why(d)) return fail(GM_EINVAL, "%s", why);
    bool fits = false;
    int rc = plan_c4_ranked(d, max_table_bytes, out, &fits);
    if (rc) return rc;
    if (!fits) return fail(GM_EFULL, "ranked table needs %llu bytes", (unsigned long long)out->table_bytes);
    return 0;
  }
  if (rank_wanted(d, flags)) {  // toot-and-otto: positions at computed indices (gm_ranked.h)
    bool fits = false;
    int rc = plan_ranked(d, max_table_bytes, out, &fits);
    if (rc) return rc;
    if (fits) return 0;
    memset(out, 0, sizeof *out);
    out->max_levels = (uint32_t)d->max_levels;
    out->scratch_bytes = scratch_bytes_for(d->max_levels);
  }
  if (positions == 0) {
    gm_game_info(game, &positions, nullptr, nullptr);
    if (positions == 0) return fail(GM_EINVAL, "no known position bound for this board; pass an estimate");
  }
  if (bk_ok(d) && !(flags & GM_F_HASH_TABLE)) {
    // bucketed levels: keys (levels buffer), words + in-edges + two
    // partition buffers of the widest level's in-edges (table buffer)
    const u64 P = positions + 64, E = bk_edges_bound(d, positions), Em = bk_emax_bound(E);
    if (Em >= 0xFFFFFFF0ull) return fail(GM_EINVAL, "a level of more than 2^32 edges: not supported");
    const u64 bytes = bk_fixed_bytes(P, E, 1) + 24 * Em;  // words, in-edges (u32 parent + u16 child), staging
    // over the caller's byte budget: the keyed hash table instead (as a
    // dense table over budget falls back above)
    if (max_table_bytes == 0 || bytes <= max_table_bytes) {
      out->mode = GM_MODE_BUCKETED;
      out->level_capacity = P;
      out->table_slots = E;
      out->table_bytes = bytes;
      out->scratch_bytes = bk_scratch(d->max_levels).end;
      return 0;
    }
  }
  uint64_t slots = 1024;
  while (slots < 2 * positions) slots <<= 1;  // load factor <= 0.5
  out->mode = GM_MODE_HASHED;
  out->table_slots = slots;
  out->table_bytes = slots * sizeof(gm_slot);
  out->level_capacity = positions + 64;
  return 0;
}

int gm_plan_keyed_shard(int game, int rank, int world, uint64_t positions, uint32_t flags, uint64_t max_table_bytes,
                        gm_plan_t* out) {
  const Desc* d = get_game(game);
  if (!d || !out) return fail(GM_EINVAL, "bad argument");
  if (world < 2 || world > 8 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad shard %d/%d (2..8 ranks)", rank, world);
  if (flags & GM_F_RANKED_SHARD) {  // the RANKED index space, md5-owned slots (gm_ranked_shard.h)
    memset(out, 0, sizeof *out);
    if (d->bsym) return fail(GM_EINVAL, "board_symmetry=1 has no ranked layout: the RANKED index has no representative form");
    if (d->kind == K_CONNECT)
      return fail(GM_EINVAL, "md5 shards of the RANKED layout serve toot-and-otto boards only (connect four: one GPU)");
    return plan_ranked_shard(d, world, max_table_bytes, out);
  }
  if (!bk_ok(d) || (flags & GM_F_HASH_TABLE))
    return fail(GM_EINVAL, "md5-sharded bucketed levels need every move to advance one level");
  memset(out, 0, sizeof *out);
  out->max_levels = (uint32_t)d->max_levels;
  if (positions == 0) {
    gm_game_info(game, &positions, nullptr, nullptr);
    if (positions == 0) return fail(GM_EINVAL, "no known position bound for this board; pass an estimate");
  }
  const u64 P = positions + 64, E = bk_shard_edges_bound(d, positions), Em = bk_emax_bound(E);
  if (Em >= 0xFFFFFFF0ull) return fail(GM_EINVAL, "a level of more than 2^32 edges: not supported");
  const u64 bytes = bk_fixed_bytes(P, E, 2) + 48 * Em + 64;  // the one-GPU layout + local in-edges + the exchange buffers
  if (max_table_bytes && bytes > max_table_bytes)
    return fail(GM_EFULL, "bucketed shard needs %llu bytes", (unsigned long long)bytes);
  out->mode = GM_MODE_BUCKETED;
  out->level_capacity = P;
  out->table_slots = E;
  out->table_bytes = bytes;
  out->scratch_bytes = bk_scratch(d->max_levels).end;
  return 0;
}

int gm_solver_create_shard(int game, int rank, int world, const gm_buffers* buf, gm_solver** out) {
  const Desc* d = get_game(game);
  if (!d || !buf || !out) return fail(GM_EINVAL, "bad argument");
  if (!buf->table || !buf->scratch) return fail(GM_EINVAL, "null device buffer");
  if (buf->scratch_bytes < scratch_bytes_for(d->max_levels)) return fail(GM_EINVAL, "scratch too small (use gm_plan)");
  DenseGeom g;
  memset(&g, 0, sizeof g);
  if (buf->mode == GM_MODE_DENSE) {
    if (!d->dense_ok) return fail(GM_EINVAL, "game has no dense layout");
    int rc = dense_geom(d, rank, world, &g);
    if (rc) return rc;
    if (buf->table_slots != (u64)d->max_levels * g.v.Wl) return fail(GM_EINVAL, "dense table must hold levels * Wl words (use gm_plan_shard)");
    // the word width follows from the flags: a table planned with 16-bit
    // words is too small for the 32-bit kernels other flags select
    const u64 need = dense_words_bytes(d, g, dense_plan_bits(d, world, buf->flags)) + dense_bits_bytes(d, g);
    if (buf->table_bytes < need)
      return fail(GM_EINVAL, "dense table of %llu bytes, these flags need %llu (plan with the flags the solver is "
                             "created with)", (unsigned long long)buf->table_bytes, (unsigned long long)need);
  } else if (buf->mode == GM_MODE_PLANES) {
    if (!d->dense_ok || !plane_ok(d, world)) return fail(GM_EINVAL, "game has no planes layout");
    if (world > 1 && (rank < 0 || rank >= world)) return fail(GM_EINVAL, "bad shard %d/%d", rank, world);
  } else if (buf->mode == GM_MODE_RANKED) {
    if (world != 1 && !(buf->flags & GM_F_RANKED_SHARD))
      return fail(GM_EINVAL, "ranked md5 shards are planned with GM_F_RANKED_SHARD (gm_plan_keyed_shard)");
    if (world > 8 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad ranked shard %d/%d (2..8 ranks)", rank, world);
    if (d->bsym) return fail(GM_EINVAL, "board_symmetry=1 has no ranked layout: the RANKED index has no representative form");
    if (d->kind == K_CONNECT) {
      if (world != 1) return fail(GM_EINVAL, "the RANKED layout of connect four runs on one GPU");
      if (const char* why = c4_rank_why(d)) return fail(GM_EINVAL, "%s", why);
    } else if (!rank_ok(d)) {
      return fail(GM_EINVAL, "game has no ranked layout");
    }
  } else if (buf->mode == GM_MODE_BUCKETED) {
    if (world < 1 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad shard %d/%d", rank, world);
    if (world > 8) return fail(GM_EINVAL, "md5-sharded bucketed levels support up to 8 ranks");
    if (!bk_ok(d)) return fail(GM_EINVAL, "bucketed levels need every move to advance one level");
    if (!buf->levels || buf->level_capacity < 2) return fail(GM_EINVAL, "null level store");
    if (buf->scratch_bytes < bk_scratch(d->max_levels).end) return fail(GM_EINVAL, "scratch too small (use gm_plan)");
    const u64 fixed = bk_fixed_bytes(buf->level_capacity, buf->table_slots, world);
    if (buf->table_bytes < fixed + (world > 1 ? 48 : 24) * 1024ull)
      return fail(GM_EINVAL, "bucketed table too small (use gm_plan / gm_plan_keyed_shard)");
  } else if (buf->mode == GM_MODE_HASHED) {
    if (world < 1 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad shard %d/%d", rank, world);
    if (!buf->levels || buf->level_capacity < 1) return fail(GM_EINVAL, "null level store");
    if (buf->table_slots < 2 || (buf->table_slots & (buf->table_slots - 1)))
      return fail(GM_EINVAL, "table_slots must be a power of two");
    if (buf->table_bytes < buf->table_slots * sizeof(gm_slot))
      return fail(GM_EINVAL, "keyed table of %llu bytes holds fewer than %llu slots",
                  (unsigned long long)buf->table_bytes, (unsigned long long)buf->table_slots);
  } else {
    return fail(GM_EINVAL, "unknown mode %u", buf->mode);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GM_ENOGPU, "no HIP device");
  gm_solver* s = new gm_solver();
  s->d = *d;
  s->mode = buf->mode;
  s->words = (uint32_t*)buf->table;
  s->nslots = buf->table_slots;
  s->view = g.v;
  s->plan_bits = buf->mode == GM_MODE_DENSE ? dense_plan_bits(d, world, buf->flags) : 32;
  s->bits = (u64*)((char*)buf->table + (buf->mode == GM_MODE_DENSE ? dense_words_bytes(d, g, s->plan_bits) : 0));
  s->rank = rank;
  s->world = world;
  s->nblocks = g.nblocks;
  s->comm = nullptr;
  s->tab = (gm_slot*)buf->table;
  s->mask = buf->table_slots - 1;
  s->lv = (u64*)buf->levels;
  s->lcap = buf->level_capacity;
  s->st = (DevState*)buf->scratch;
  s->masks = (const u64*)((char*)buf->scratch + mask_tables_offset(d->max_levels));
  s->bcount = (BlockCount*)((char*)buf->scratch + count_slots_offset(d->max_levels));
  s->flags = buf->flags;
  s->grid = launch_grid();
  if (buf->stream) {
    s->stream = (hipStream_t)buf->stream;
    s->own_stream = false;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete s;
      return fail(GM_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    s->own_stream = true;
  }
  int rc = 0;
  switch (s->mode) {
    case GM_MODE_DENSE: rc = dense_setup(s, buf); break;
    case GM_MODE_BUCKETED: bk_setup(s, buf); break;
    case GM_MODE_PLANES: rc = plane_setup(s, buf); break;
    case GM_MODE_RANKED: rc = d->kind == K_CONNECT ? c4_setup(s, buf) : rank_setup(s, buf); break;
    default: break;  // HASHED: the common fields are all of it
  }
  if (rc) {  // (fail()'s message stands: gm_solver_destroy sets none)
    gm_solver_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}


int gm_solver_create(int game, const gm_buffers* buf, gm_solver** out) {
  return gm_solver_create_shard(game, 0, 1, buf, out);
}

int gm_comm_unique_id(void* id_out) {
  if (!id_out) return fail(GM_EINVAL, "null argument");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return fail(GM_EHIP, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  memcpy(id_out, &id, sizeof id);
  return 0;
}

int gm_solver_comm_init(gm_solver* s, const void* id) {
  if (!s || !id) return fail(GM_EINVAL, "bad argument");
  if (s->world <= 1) return 0;
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  ncclComm_t c;
  ncclResult_t r = ncclCommInitRank(&c, s->world, uid, s->rank);
  if (r != ncclSuccess) return fail(GM_EHIP, "ncclCommInitRank: %s", ncclGetErrorString(r));
  s->comm = c;
  if (!s->errg && hipMalloc((void**)&s->errg, (size_t)s->world * sizeof(u64)) != hipSuccess)
    return fail(GM_EHIP, "error-mask gather buffer");
  return 0;
}

int gm_shard_halo_sigs(int game, int rank, int world, uint32_t flags, uint64_t* out, uint32_t levels) {
  (void)flags;  // the halo geometry does not depend on the kernel families
  const Desc* d = get_game(game);
  if (!d || !out || world < 1 || rank < 0 || rank >= world) return fail(GM_EINVAL, "bad argument");
  if (!d->dense_ok) return fail(GM_EINVAL, "game has no dense layout");
  if (levels < (uint32_t)d->max_levels) return fail(GM_EINVAL, "out holds %u levels, the game has %d", levels, d->max_levels);
  std::unique_ptr<gm_solver> s(new gm_solver());
  int rc = shard_host_geom(d, rank, world, s.get());
  if (rc) return rc;
  for (int L = 0; L < d->max_levels; L++) halo_sigs(s.get(), (u64)L, (u64*)out + (size_t)L * 4);
  return 0;
}

int gm_solver_set_transport(gm_solver* s, gm_xfer_fn fn, void* ctx) {
  if (!s) return fail(GM_EINVAL, "bad argument");
  if ((s->mode != GM_MODE_DENSE && s->mode != GM_MODE_PLANES && s->mode != GM_MODE_BUCKETED &&
       s->mode != GM_MODE_RANKED) || s->world <= 1)
    return fail(GM_EINVAL, "a transport serves dense / planes / bucketed / ranked shards of a world > 1");
  s->xfer = fn;
  s->xfer_ctx = ctx;
  return 0;
}

// an opened tablebase file (gm_solver_open_table) is read, never solved
static int table_file_refuses(const char* what) {
  return fail(GM_EINVAL, "%s: the solver is an opened tablebase file (gm_solver_open_table): it serves the readers "
                         "only -- no solve, no steps, no flags", what);
}

int gm_solver_set_steps(gm_solver* s, uint32_t first, uint32_t stop) {
  if (!s) return fail(GM_EINVAL, "bad argument");
  if (s->mode == GM_MODE_FILE) return table_file_refuses("gm_solver_set_steps");
  const uint32_t n = 2u * (uint32_t)s->d.max_levels;
  if (s->world > 1) return fail(GM_EINVAL, "stop/resume drives one-GPU solves only");
  if (first > n || (stop && (stop <= first || stop > n))) return fail(GM_EINVAL, "bad step range [%u, %u) of %u", first, stop, n);
  s->step_first = first;
  s->step_stop = stop;
  return 0;
}

int gm_solver_set_flags(gm_solver* s, uint32_t flags) {
  if (!s) return fail(GM_EINVAL, "null solver");
  if (s->mode == GM_MODE_FILE) return table_file_refuses("gm_solver_set_flags");
  if ((flags & ~GM_F_KERNEL_TIMING) != (s->flags & ~GM_F_KERNEL_TIMING))
    return fail(GM_EINVAL, "only GM_F_KERNEL_TIMING changes after creation: the kernel families and word width "
                           "are fixed by the flags the solver was planned and created with");
  s->flags = flags;
  return 0;
}

void gm_solver_destroy(gm_solver* s) {
  if (!s) return;
  for (hipEvent_t e : s->pev) (void)hipEventDestroy(e);
  if (s->gfwd) (void)hipGraphExecDestroy(s->gfwd);
  if (s->gbwd) (void)hipGraphExecDestroy(s->gbwd);
  for (hipEvent_t e : s->pse)
    if (e) (void)hipEventDestroy(e);
  for (PlaneSlot& q : s->pring) {
    for (hipEvent_t e : q.ev)
      if (e) (void)hipEventDestroy(e);
    if (q.host) (void)hipHostFree(q.host);
  }
  if (s->phost) (void)hipHostFree(s->phost);
  if (s->cstream) (void)hipStreamDestroy(s->cstream);
  if (s->cstream2) (void)hipStreamDestroy(s->cstream2);
  if (s->comm2) (void)ncclCommDestroy(s->comm2);
  if (s->comm) (void)ncclCommDestroy(s->comm);
  if (s->errg) (void)hipFree(s->errg);
  if (s->xdev) (void)hipFree(s->xdev);
  if (s->rlv_dev) (void)hipFree(s->rlv_dev);
  if (s->c4_dev) (void)hipFree(s->c4_dev);
  if (s->cen_dev) (void)hipFree(s->cen_dev);
  if (s->exp_dev) (void)hipFree(s->exp_dev);
  if (s->xgeo_dev) (void)hipFree(s->xgeo_dev);
  delete s->tb;
  delete s->tk;
  if (s->own_stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// Queued one-table PLANES solves: enqueue without waiting, collect later
// (in order).  Solves queued back to back run back to back on the solver's
// stream with no host round trip between them.
int gm_solver_solve_async(gm_solver* s, uint64_t* ticket) {
  if (!s || !ticket) return fail(GM_EINVAL, "bad argument");
  if (s->mode != GM_MODE_PLANES || s->world > 1) return fail(GM_EINVAL, "queued solves: one-table PLANES solvers only");
  if (s->pq_next - s->pq_done >= (u64)kPlaneRing)
    return fail(GM_EINVAL, "%d solves queued: collect one first", kPlaneRing);
  const u64 t = s->pq_next;
  s->solved = false;
  gm_result scratch;
  memset(&scratch, 0, sizeof scratch);
  const int rc = run_planes({s}, &scratch, true);
  if (rc) return rc;
  *ticket = t;
  return 0;
}

int gm_solver_collect(gm_solver* s, uint64_t ticket, gm_result* out) {
  if (!s || !out) return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  if (s->mode != GM_MODE_PLANES || s->world > 1) return fail(GM_EINVAL, "queued solves: one-table PLANES solvers only");
  const int rc = plane_collect(s, ticket, out);
  s->solved = rc == 0 && s->pq_done == s->pq_next;  // (no later solve is rewriting the table)
  return rc;
}

// the solve of one solver, or of the shards of an in-process group, by layout
static int solve_by_mode(const std::vector<gm_solver*>& ss, gm_result* out) {
  gm_solver* s = ss[0];
  if (s->mode == GM_MODE_DENSE) return run_dense(ss, out);
  if (s->mode == GM_MODE_PLANES) return run_planes(ss, out);
  if (s->mode == GM_MODE_RANKED) return s->world > 1 ? run_ranked_shards(ss, out) : run_ranked(s, out);
  if (s->mode == GM_MODE_BUCKETED) return s->world > 1 ? run_bucketed_shards(ss, out) : solve_bucketed(s, out);
  if (s->world > 1) return fail(GM_EINVAL, "keyed-table shard %d/%d: drive it with gm_ks_* (md5 exchange)", s->rank, s->world);
  return run_hashed(s, out);
}

int gm_solver_solve(gm_solver* s, gm_result* out) {
  if (!s || !out) return fail(GM_EINVAL, "bad argument");
  if (s->mode == GM_MODE_FILE) return table_file_refuses("gm_solver_solve");
  s->solved = false;
  memset(out, 0, sizeof *out);
  const int rc = solve_by_mode({s}, out);
  s->solved = rc == 0;  // (GM_PARTIAL: stopped early, the table is not finished)
  return rc;
}

int gm_solve_group(gm_solver** shards, int n, gm_result* out) {
  if (!shards || n < 1 || !out) return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  std::vector<gm_solver*> ss(shards, shards + n);
  for (gm_solver* s : ss)
    if (!s) return fail(GM_EINVAL, "null shard");
  for (gm_solver* s : ss)
    if (s->mode == GM_MODE_FILE) return table_file_refuses("gm_solve_group");
  for (gm_solver* s : ss) s->solved = false;
  // a group's BUCKETED shards take the sharded loop whatever their world, and
  // keyed tables meet the dense loop's group checks; the rest is one dispatch
  const uint32_t mode = ss[0]->mode;
  const int rc = mode == GM_MODE_BUCKETED ? run_bucketed_shards(ss, out)
                 : mode == GM_MODE_HASHED ? run_dense(ss, out)
                                          : solve_by_mode(ss, out);
  for (gm_solver* s : ss) s->solved = rc == 0;
  return rc;
}

#include "gm_table.h"
#include "gm_moves.h"

int gm_solver_moves(gm_solver* s, const uint64_t* keys_dev, uint64_t n, uint64_t* children_dev, uint32_t* words_dev,
                    uint8_t* nchild_dev, int8_t* best_dev) {
  if (!s || (n && (!keys_dev || !children_dev || !words_dev || !nchild_dev || !best_dev)))
    return fail(GM_EINVAL, "bad argument");
  const int rc = moves_ready(s, "gm_solver_moves");
  if (rc || !n) return rc;
  return moves_run(s, keys_dev, n, children_dev, words_dev, nchild_dev, best_dev);
}

int gm_solver_line(gm_solver* s, uint64_t key, uint64_t* keys_dev, uint32_t* words_dev, uint64_t cap, uint64_t* n) {
  if (!s || !n || (cap && (!keys_dev || !words_dev))) return fail(GM_EINVAL, "bad argument");
  *n = 0;
  const int rc = moves_ready(s, "gm_solver_line");
  if (rc || !cap) return rc;
  return line_run(s, key, keys_dev, words_dev, cap, n);
}

int gm_solver_audit(gm_solver* s, uint64_t* bad_keys_dev, uint64_t cap, uint64_t out[4]) {
  if (!s || !out || (cap && !bad_keys_dev)) return fail(GM_EINVAL, "bad argument");
  const int rc = moves_ready(s, "gm_solver_audit");
  if (rc) return rc;
  return audit_run(s, bad_keys_dev, cap, out);
}

#include "gm_census.h"

int gm_solver_census(gm_solver* s, uint32_t how, uint64_t* by_rem_dev, uint32_t rem_bins, uint64_t* by_level_dev,
                     uint32_t levels, uint64_t extremes[12]) {
  if (!s || !by_rem_dev || (how & ~GM_CENSUS_GENERIC) || (!by_level_dev && levels) || rem_bins == 0xFFFFFFFFu)
    return fail(GM_EINVAL, "bad argument");
  const int rc = moves_ready(s, "gm_solver_census");
  if (rc) return rc;
  if (by_level_dev && levels < (uint32_t)s->d.max_levels)
    return fail(GM_EINVAL, "gm_solver_census: %u level rows, the game has %d", levels, s->d.max_levels);
  return census_run(s, how, by_rem_dev, rem_bins, by_level_dev, levels, extremes);
}

#include "gm_export.h"

// gm_host_expand through the instantiation the bucketed kernels run for this
// descriptor (fixed_kind: a compile-time board where one exists, symmetric
// where the descriptor asks), so that both forms can be compared on the host
int gm_host_expand_fixed(int game, const uint64_t* keys, size_t n, uint64_t* children, uint8_t* nchild, uint8_t* prim) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !children || !nchild || !prim))) return fail(GM_EINVAL, "bad argument");
  if (!bk_ok(d)) return fail(GM_EINVAL, "the game has no bucketed kernels");
  bool over = false;
  bk_dispatch(*d, [&](auto kind_) {
    constexpr int K_ = decltype(kind_)::value;
    for (size_t i = 0; i < n; i++) {
      prim[i] = (uint8_t)Game<K_>::prim(*d, keys[i]);
      int c = 0;
      if (prim[i] == UNDECIDED)
        Game<K_>::children(*d, keys[i], [&](uint64_t ck, int) {
          if (c < GM_MAXCHILD) children[i * GM_MAXCHILD + c] = ck;
          c++;
        });
      over |= c > GM_MAXCHILD;
      nchild[i] = (uint8_t)c;
    }
  });
  if (over) return fail(GM_ECORRUPT, "more than %d children", GM_MAXCHILD);
  return 0;
}

int gm_tb_info(int game, uint64_t* index_space) {
  const Desc* d = get_game(game);
  if (!d || !index_space) return fail(GM_EINVAL, "bad argument");
  u64 space = 0;
  const int rc = tb_space(d, &space, nullptr);
  if (!rc) *index_space = space;
  return rc;
}

int gm_tb_index(int game, const uint64_t* keys, size_t n, uint64_t* index) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !index))) return fail(GM_EINVAL, "bad argument");
  u64 space;
  RankShape rs;
  const int rc = tb_space(d, &space, &rs);
  if (rc) return rc;
  if (d->kind == K_SUM) {
    const u64 total = tb_sum_total(d);
    for (size_t i = 0; i < n; i++) index[i] = tb_sum_index(total, keys[i]);
    return 0;
  }
  rs.g.base = rs.base.data();  // (the host's copy: rk_slot_of reads nothing else through a pointer)
  for (size_t i = 0; i < n; i++) {
    u64 slot;
    uint32_t L;
    index[i] = rk_slot_of(rs.g, keys[i], &slot, &L) ? slot : GM_NO_INDEX;
  }
  return 0;
}

int gm_ranked_slots(int game, const uint64_t* keys, size_t n, uint64_t* slots, uint32_t* levels) {
  const Desc* d = get_game(game);
  if (!d || (n && (!keys || !slots || !levels))) return fail(GM_EINVAL, "bad argument");
  if (d->bsym) return fail(GM_EINVAL, "board_symmetry=1 has no ranked layout: the RANKED index has no representative form");
  auto each = [&](auto&& slot_of) {
    for (size_t i = 0; i < n; i++) {
      u64 slot;
      uint32_t L;
      const bool ok = slot_of(keys[i], &slot, &L);
      slots[i] = ok ? slot : GM_NO_INDEX;
      levels[i] = ok ? L : 0xFFFFFFFFu;
    }
  };
  if (d->kind == K_CONNECT) {
    if (const char* why = c4_rank_why(d)) return fail(GM_EINVAL, "%s", why);
    C4Shape cs;
    c4_shape(d, &cs);
    c4_host_geom(&cs);
    each([&](u64 key, u64* slot, uint32_t* L) { return c4_slot_of(cs.g, key, slot, L); });
    return 0;
  }
  if (!rank_ok(d)) return fail(GM_EINVAL, "game has no ranked layout (toot-and-otto and connect four boards have one)");
  RankShape rs;
  const int rc = rank_shape(d, &rs);
  if (rc) return rc;
  rs.g.base = rs.base.data();
  each([&](u64 key, u64* slot, uint32_t* L) { return rk_slot_of(rs.g, key, slot, L); });
  return 0;
}

int gm_solver_export(gm_solver* s, uint32_t how, uint64_t first, uint64_t count, uint32_t word_bytes,
                     uint64_t* bits_dev, uint32_t* block_counts_dev, void* words_dev, uint64_t words_cap,
                     uint64_t* n_words) {
  if (!s || !n_words || (how & ~GM_EXPORT_GENERIC) || (word_bytes != 1 && word_bytes != 2 && word_bytes != 4) ||
      (count && (!bits_dev || !block_counts_dev)) || (words_cap && !words_dev) || (((uintptr_t)words_dev | (uintptr_t)bits_dev) & 15u))
    return fail(GM_EINVAL, "bad argument");
  *n_words = 0;
  int rc = moves_ready(s, "gm_solver_export");
  if (rc) return rc;
  u64 space;
  rc = tb_space(&s->d, &space, nullptr);
  if (rc) return rc;
  if (first % GM_TB_BLOCK || count % GM_TB_BLOCK || first > space || count > space - first)
    return fail(GM_EINVAL, "gm_solver_export: indexes [%llu, +%llu) are no whole blocks of %u inside the index space %llu",
                (unsigned long long)first, (unsigned long long)count, GM_TB_BLOCK, (unsigned long long)space);
  if (!count) return 0;
  return export_run(s, how, first, count, word_bytes, (u64*)bits_dev, block_counts_dev, words_dev, words_cap, n_words);
}

#include "gm_export_keyed.h"

int gm_mix64(const uint64_t* keys, size_t n, uint64_t* out) {
  if (n && (!keys || !out)) return fail(GM_EINVAL, "bad argument");
  for (size_t i = 0; i < n; i++) out[i] = mix64(keys[i]);
  return 0;
}

int gm_solver_export_keyed(gm_solver* s, uint32_t how, uint32_t bucket_bits, uint32_t word_bytes, void* stage_dev,
                           uint64_t* dir_dev, void* keys_dev, void* words_dev, uint64_t cap, uint64_t out[4]) {
  if (!s || !out || !dir_dev || (how & ~GM_EXPORT_GENERIC) || bucket_bits > 32 ||
      (word_bytes != 1 && word_bytes != 2 && word_bytes != 4) || (cap && (!stage_dev || !keys_dev || !words_dev)) ||
      (((uintptr_t)keys_dev | (uintptr_t)words_dev) & 15u) || (((uintptr_t)stage_dev | (uintptr_t)dir_dev) & 7u))
    return fail(GM_EINVAL, "bad argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  const int rc = moves_ready(s, "gm_solver_export_keyed");
  if (rc) return rc;
  return export_keyed_run(s, how, bucket_bits, word_bytes, stage_dev, (u64*)dir_dev, keys_dev, words_dev, cap, out);
}

int gm_solver_query(gm_solver* s, const uint64_t* keys_dev, uint64_t n, uint32_t* words_dev) {
  if (!s || (n && (!keys_dev || !words_dev))) return fail(GM_EINVAL, "bad argument");
  if (!n) return 0;
  return query_run(s, keys_dev, n, words_dev);
}

int gm_solver_positions(gm_solver* s, uint64_t* keys_dev, uint64_t cap, uint64_t* n) {
  if (!s || !n) return fail(GM_EINVAL, "bad argument");
  return positions_run(s, keys_dev, cap, n);
}

int gm_solver_checksum(gm_solver* s, uint64_t out[6]) {
  if (!s || !out) return fail(GM_EINVAL, "bad argument");
  return checksum_run(s, out);
}

#define GM_TABLE_FILE_HOST 1
#include "gm_table_file.h"

int gm_table_check(int game, const void* header, uint64_t header_bytes, uint64_t file_bytes, uint64_t out[12]) {
  const Desc* d = get_game(game);
  if (!d || !header || !out) return fail(GM_EINVAL, "bad argument");
  TfInfo fi;
  const int rc = table_check(d, (const uint8_t*)header, header_bytes, file_bytes, &fi);
  if (rc) return rc;
  const uint64_t v[12] = {fi.format,    fi.positions, fi.wb,  fi.kb,        fi.b,
                          fi.space,     fi.off0,      fi.off1, fi.words_off,
                          (scratch_bytes_for(d->max_levels) + 255) / 256 * 256 + fi.index_bytes, fi.index_bytes, 0};
  memcpy(out, v, sizeof v);
  return 0;
}

int gm_solver_open_table(int game, const void* image_dev, uint64_t bytes, void* scratch_dev, uint64_t scratch_bytes,
                         void* stream, gm_solver** out) {
  const Desc* d = get_game(game);
  if (!d || !image_dev || !scratch_dev || !out) return fail(GM_EINVAL, "bad argument");
  *out = nullptr;
  return table_open(d, image_dev, bytes, scratch_dev, scratch_bytes, stream, out);
}

// gm_solve keeps its solver per game id until the next gm_solve of that game
// or gm_release(game), so gm_query(game, ...) reads the table it left in the
// caller's buffers (SURVEY §8b's one-shot pair)
static std::mutex g_solved_mu;
static std::map<int, gm_solver*> g_solved;

// gm_solve over several GPUs of this process (SURVEY §8b's `ngpus`; the
// reference's `mpiexec -n P`, solver_launcher.py:30,76-84): shard i of the
// plan gm_plan_multi gives lives on device i in buf[i]; one RCCL
// communicator per device (ncclCommInitAll) and one host thread per device
// driving its shard's gm_solver_solve -- the halo rows (PLANES / DENSE) and
// the md5 all-to-alls (BUCKETED) are RCCL calls every rank's thread must
// enter.  Every rank ends with the job's totals and root word.
struct MultiSolve {
  std::vector<gm_solver*> ss;
};
static std::map<int, MultiSolve> g_multi;  // under g_solved_mu

static void multi_destroy(MultiSolve& m) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (size_t i = 0; i < m.ss.size(); i++)
    if (m.ss[i]) {
      (void)hipSetDevice((int)i);
      gm_solver_destroy(m.ss[i]);
      m.ss[i] = nullptr;
    }
  (void)hipSetDevice(cur);
}

// Failure in bounded time: every early return goes through bail (shards and
// communicators freed, the caller's device restored).  A shard whose solve
// fails on its own side defers the error to the end-of-solve reduction (the
// staged PLANES backward, the md5 BUCKETED levels), so its peers finish; a
// shard whose solve returns while its peers may still wait in an RCCL call
// (an early return) aborts EVERY communicator of the group (ncclCommAbort:
// the peers' pending calls return with an error), so join() always returns.
static int solve_multi(int game, int ngpus, const gm_buffers* buf, gm_result* out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
  if (ngpus > ndev) return fail(GM_EINVAL, "ngpus %d: %d GPU(s) visible", ngpus, ndev);
  for (int i = 0; i < ngpus; i++)
    if (buf[i].mode != buf[0].mode) return fail(GM_EINVAL, "buf[%d]: every shard needs the mode of gm_plan_multi", i);
  int cur = 0;
  HIPCHK(hipGetDevice(&cur));
  MultiSolve m;
  m.ss.assign((size_t)ngpus, nullptr);
  std::vector<ncclComm_t> comms((size_t)ngpus, nullptr);
  std::vector<int> devs((size_t)ngpus);
  for (int i = 0; i < ngpus; i++) devs[(size_t)i] = i;
  bool aborted = false;  // every communicator aborted (and detached from its shard)
  auto bail = [&](int rc) {
    if (!aborted)
      for (size_t i = 0; i < comms.size(); i++)
        if (comms[i] && !(m.ss[i] && m.ss[i]->comm == comms[i])) (void)ncclCommDestroy(comms[i]);
    multi_destroy(m);
    (void)hipSetDevice(cur);
    return rc;
  };
  for (int i = 0; i < ngpus; i++) {
    if (hipSetDevice(i) != hipSuccess) return bail(fail(GM_EHIP, "hipSetDevice(%d)", i));
    const int rc = gm_solver_create_shard(game, i, ngpus, &buf[i], &m.ss[(size_t)i]);
    if (rc) return bail(fail(rc, "shard %d: %s", i, gm_last_error()));
  }
  const ncclResult_t r = ncclCommInitAll(comms.data(), ngpus, devs.data());
  if (r != ncclSuccess) return bail(fail(GM_EHIP, "ncclCommInitAll: %s", ncclGetErrorString(r)));
  for (int i = 0; i < ngpus; i++) {
    gm_solver* sh = m.ss[(size_t)i];
    sh->comm = comms[(size_t)i];
    if (hipSetDevice(i) != hipSuccess) return bail(fail(GM_EHIP, "hipSetDevice(%d)", i));
    if (!sh->errg && hipMalloc((void**)&sh->errg, (size_t)ngpus * sizeof(u64)) != hipSuccess)
      return bail(fail(GM_EHIP, "error-mask gather buffer"));
  }
  // The staged PLANES deal sends its odd-direction halos on a second
  // communicator per shard (gm_plane_run.h): split here, before any shard
  // thread runs, one group call over every rank -- so abort_all below knows
  // every communicator a thread can wait in (a shard that split its own on
  // first use could be blocked in comm2 while the abort missed it).
  bool staged_deal = false;
  for (gm_solver* sh : m.ss) staged_deal = staged_deal || (sh->mode == GM_MODE_PLANES && sh->pstage_k);
  if (staged_deal) {
    ncclResult_t r1 = ncclGroupStart();
    for (int i = 0; i < ngpus && r1 == ncclSuccess; i++) {
      gm_solver* sh = m.ss[(size_t)i];
      if (!sh->comm2) r1 = ncclCommSplit(sh->comm, 0, sh->rank, &sh->comm2, nullptr);
    }
    const ncclResult_t r2 = ncclGroupEnd();
    if (r1 != ncclSuccess || r2 != ncclSuccess)
      return bail(fail(GM_EHIP, "ncclCommSplit (staged deal): %s", ncclGetErrorString(r1 != ncclSuccess ? r1 : r2)));
  }
  std::vector<gm_result> res((size_t)ngpus);
  std::vector<int> rcs((size_t)ngpus, 0);
  std::vector<std::string> msg((size_t)ngpus);
  std::mutex abort_mu;  // one abort of the whole group, by the first thread that fails
  std::atomic<int> gabort{0};
  for (gm_solver* sh : m.ss) sh->gabort = &gabort;
  auto abort_all = [&]() {
    std::lock_guard<std::mutex> lk(abort_mu);
    if (aborted) return;
    aborted = true;
    // published first: a shard that checks it (RCCL_LIVE, before every RCCL
    // call) issues nothing more on these communicators; then every one of
    // them -- the primary ones and the staged deal's second ones -- is
    // aborted, so a peer waiting in any RCCL call on any of them returns
    gabort.store(1, std::memory_order_release);
    for (size_t i = 0; i < comms.size(); i++)
      if (comms[i]) (void)ncclCommAbort(comms[i]);
    for (gm_solver* sh : m.ss)
      if (sh && sh->comm2) (void)ncclCommAbort(sh->comm2);
  };
  std::vector<std::thread> th;
  for (int i = 0; i < ngpus; i++)
    th.emplace_back([&, i]() {
      if (hipSetDevice(i) != hipSuccess) {
        rcs[(size_t)i] = GM_EHIP;
        msg[(size_t)i] = "hipSetDevice";
        abort_all();
        return;
      }
      rcs[(size_t)i] = gm_solver_solve(m.ss[(size_t)i], &res[(size_t)i]);
      if (rcs[(size_t)i]) {
        msg[(size_t)i] = gm_last_error();
        // a deferred failure has already taken every peer through the
        // reduction; any other failure may leave them waiting: abort
        if (!m.ss[(size_t)i]->defer_rc) abort_all();
      }
    });
  for (auto& t : th) t.join();
  (void)hipSetDevice(cur);
  for (gm_solver* sh : m.ss) sh->gabort = nullptr;
  if (aborted)  // the aborted communicators are not destroyed again with the shards
    for (gm_solver* sh : m.ss)
      if (sh) sh->comm = sh->comm2 = nullptr;
  for (int i = 0; i < ngpus; i++)
    if (rcs[(size_t)i]) return bail(fail(rcs[(size_t)i], "shard %d: %s", i, msg[(size_t)i].c_str()));
  *out = res[0];
  std::lock_guard<std::mutex> lk(g_solved_mu);
  g_multi[game] = std::move(m);
  return 0;
}

int gm_plan_multi(int game, int ngpus, uint64_t positions, uint32_t flags, uint64_t max_table_bytes,
                  gm_plan_t* plans) {
  const Desc* d = get_game(game);
  if (!d || !plans || ngpus < 1) return fail(GM_EINVAL, "bad argument");
  if (ngpus == 1) return gm_plan(game, positions, flags, max_table_bytes, plans);
  if (d->dense_ok) {  // sum games: PLANES (or level-major DENSE) blocks of the last heap
    for (int r = 0; r < ngpus; r++) {
      const int rc = gm_plan_shard(game, r, ngpus, flags, max_table_bytes, &plans[r]);
      if (rc) return rc;
    }
    return 0;
  }
  if (!bk_ok(d)) return fail(GM_EINVAL, "%d GPUs in one process: the game needs a dense or bucketed shard layout "
                                        "(keyed games of other shapes: one process per GPU, keyed.py)", ngpus);
  if (positions == 0) {
    gm_game_info(game, &positions, nullptr, nullptr);
    if (positions == 0) return fail(GM_EINVAL, "no known position bound for this board; pass an estimate");
  }
  // the md5 shard bound of keyed._shard_bound: the share + 3 % + 64 K
  const u64 per = (u64)((double)positions * 1.03) / (u64)ngpus + 65536;
  for (int r = 0; r < ngpus; r++) {
    const int rc = gm_plan_keyed_shard(game, r, ngpus, per, flags, max_table_bytes, &plans[r]);
    if (rc) return rc;
  }
  return 0;
}

int gm_solve(int game, uint64_t root, int ngpus, const gm_buffers* buf, gm_result* out) {
  const Desc* d = get_game(game);
  if (!d) return fail(GM_EINVAL, "bad game id %d", game);
  if (ngpus < 1 || !buf || !out) return fail(GM_EINVAL, "bad argument");
  if (root != d->root) return fail(GM_EINVAL, "root must be the game's initial position");
  (void)gm_release(game);
  if (ngpus > 1) return solve_multi(game, ngpus, buf, out);
  gm_solver* s = nullptr;
  int rc = gm_solver_create(game, buf, &s);
  if (rc) return rc;
  rc = gm_solver_solve(s, out);
  if (rc) {
    gm_solver_destroy(s);
    return rc;
  }
  std::lock_guard<std::mutex> lk(g_solved_mu);
  g_solved[game] = s;
  return 0;
}

int gm_query(int game, const uint64_t* keys_dev, size_t n, uint32_t* words_dev) {
  gm_solver* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_solved_mu);
    auto it = g_solved.find(game);
    if (it != g_solved.end()) s = it->second;
  }
  if (!s) {
    std::lock_guard<std::mutex> lk(g_solved_mu);
    if (g_multi.count(game))
      return fail(GM_EINVAL, "game %d was solved on several GPUs: query its shards (gm_solver_query per device)", game);
    return fail(GM_EINVAL, "game %d has no finished gm_solve to query", game);
  }
  int rc = gm_solver_query(s, keys_dev, (uint64_t)n, words_dev);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

int gm_release(int game) {
  gm_solver* s = nullptr;
  MultiSolve m;
  {
    std::lock_guard<std::mutex> lk(g_solved_mu);
    auto it = g_solved.find(game);
    if (it != g_solved.end()) {
      s = it->second;
      g_solved.erase(it);
    }
    auto jt = g_multi.find(game);
    if (jt != g_multi.end()) {
      m = std::move(jt->second);
      g_multi.erase(jt);
    }
  }
  if (s) gm_solver_destroy(s);
  multi_destroy(m);
  return 0;
}

int gm_owner(int game, const uint64_t* keys_dev, uint64_t n, int world_size, uint32_t* owners_dev, void* stream) {
  const Desc* d = get_game(game);
  if (!d || world_size < 1 || (n && (!keys_dev || !owners_dev))) return fail(GM_EINVAL, "bad argument");
  if (!n) return 0;
  int grid = (int)std::min<u64>((n + kBlock - 1) / kBlock, (u64)launch_grid());
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_owner, dim3(grid), dim3(kBlock), 0, st, *d, (const u64*)keys_dev, n, (uint32_t)world_size,
                     owners_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// md5-sharded keyed tables (gm_keyed_shard.h): the host moves keys/words
// between ranks between these steps (gamesmanmpi_amd/keyed.py)
// ---------------------------------------------------------------------------
// (GM_KS_LAUNCH_PLAIN: kernels that never generate children -- k_ks_insert,
// k_ks_reduce)
#define GM_KS_LAUNCH(KERNEL, GRID, S, ...)                                                                  \
  kind_dispatch_sym<GenericKinds>((S)->d, (S)->d.kind, [&](auto kind_) {                                    \
    hipLaunchKernelGGL(KERNEL<decltype(kind_)::value>, dim3(GRID), dim3(kBlock), 0, (S)->stream, __VA_ARGS__); \
  })
#define GM_KS_LAUNCH_PLAIN(KERNEL, GRID, S, ...)                                                            \
  kind_dispatch<GenericKinds>((S)->d.kind, [&](auto kind_) {                                                \
    hipLaunchKernelGGL(KERNEL<decltype(kind_)::value>, dim3(GRID), dim3(kBlock), 0, (S)->stream, __VA_ARGS__); \
  })

static int ks_check(gm_solver* s, int level) {
  if (!s) return fail(GM_EINVAL, "null solver");
  if (s->mode != GM_MODE_HASHED) return fail(GM_EINVAL, "gm_ks_* drive keyed (HASHED) tables only");
  if (level < 0 || level >= s->d.max_levels) return fail(GM_EINVAL, "level %d out of range", level);
  return 0;
}

static int ks_grid(gm_solver* s, u64 n) {
  return (int)std::max<u64>(1, std::min<u64>((n + kBlock - 1) / kBlock, (u64)s->grid));
}

static int ks_errors(gm_solver* s) {
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(&err, &s->st->err, sizeof err, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (err) {
    bool full = err & (ERR_TABLE_FULL | ERR_LEVELS_FULL);
    return fail(full ? GM_EFULL : GM_ECORRUPT, "shard %d/%d:%s", s->rank, s->world, err_text(err).c_str());
  }
  return 0;
}

int gm_ks_begin(gm_solver* s, int root_owned) {
  int rc = ks_check(s, 0);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(s->tab, 0xFF, (s->mask + 1) * sizeof(gm_slot), s->stream));
  HIPCHK(hipMemsetAsync(s->st, 0, devstate_bytes(s->d.max_levels), s->stream));
  hipLaunchKernelGGL(k_ks_seed, dim3(1), dim3(64), 0, s->stream, s->tab, s->mask, s->lv, s->st, s->d.root,
                     root_owned ? 1 : 0);
  HIPCHK(hipGetLastError());
  return 0;
}

int gm_ks_level_size(gm_solver* s, int level, uint64_t* n) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  if (!n) return fail(GM_EINVAL, "null argument");
  LevelSeg g;
  HIPCHK(hipMemcpyAsync(&g, &s->st->seg[level], sizeof g, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n = (g.fe - g.fb) + (g.c2hi - g.c2lo);
  return 0;
}

int gm_ks_expand(gm_solver* s, int level, uint64_t* keys_dev, uint32_t* owners_dev, uint64_t cap, int world,
                 uint64_t* n) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  if (!n || world < 1 || (cap && (!keys_dev || !owners_dev))) return fail(GM_EINVAL, "bad argument");
  uint64_t width = 0;
  if ((rc = gm_ks_level_size(s, level, &width))) return rc;
  HIPCHK(hipMemsetAsync(&s->st->ks_cursor, 0, sizeof(u64), s->stream));
  GM_KS_LAUNCH(k_ks_expand, ks_grid(s, width), s, s->d, s->lv, s->lcap, s->st, level, (u64*)keys_dev, cap,
                   &s->st->ks_cursor);
  HIPCHK(hipGetLastError());
  u64 got = 0;
  HIPCHK(hipMemcpyAsync(&got, &s->st->ks_cursor, sizeof got, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n = got;
  if (got > cap) return fail(GM_EFULL, "expand of level %d emits %llu children (cap %llu)", level,
                             (unsigned long long)got, (unsigned long long)cap);
  if (got)
    hipLaunchKernelGGL(k_owner, dim3(ks_grid(s, got)), dim3(kBlock), 0, s->stream, s->d, (const u64*)keys_dev, got,
                       (uint32_t)world, owners_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int gm_ks_insert(gm_solver* s, int level, const uint64_t* keys_dev, uint64_t n) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  if (n && !keys_dev) return fail(GM_EINVAL, "null keys");
  if (n) GM_KS_LAUNCH_PLAIN(k_ks_insert, ks_grid(s, n), s, s->d, s->tab, s->mask, s->lv, s->lcap, s->st, level,
                          (const u64*)keys_dev, (u64)n);
  HIPCHK(hipGetLastError());
  return 0;
}

int gm_ks_finalize(gm_solver* s, int level) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  if (level + 1 >= s->d.max_levels) return fail(GM_EINVAL, "level %d is the last level", level);
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s->stream, s->st, level, s->lcap);
  HIPCHK(hipGetLastError());
  return ks_errors(s);
}

int gm_ks_counts(gm_solver* s, int level, uint64_t* counts_dev) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  uint64_t width = 0;
  if ((rc = gm_ks_level_size(s, level, &width))) return rc;
  if (!width) return 0;
  if (!counts_dev) return fail(GM_EINVAL, "null counts");
  GM_KS_LAUNCH(k_ks_counts, ks_grid(s, width), s, s->d, s->lv, s->lcap, s->st, level, counts_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int gm_ks_children(gm_solver* s, int level, const uint64_t* offsets_dev, uint64_t* keys_dev, uint32_t* owners_dev,
                   int world) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  uint64_t width = 0;
  if ((rc = gm_ks_level_size(s, level, &width))) return rc;
  if (!width) return 0;
  if (!offsets_dev || !keys_dev || !owners_dev || world < 1) return fail(GM_EINVAL, "bad argument");
  GM_KS_LAUNCH(k_ks_children, ks_grid(s, width), s, s->d, s->lv, s->lcap, s->st, level, offsets_dev,
                   (u64*)keys_dev, owners_dev, (uint32_t)world);
  HIPCHK(hipGetLastError());
  return 0;
}

int gm_ks_reduce(gm_solver* s, int level, const uint64_t* offsets_dev, const uint32_t* child_words_dev) {
  int rc = ks_check(s, level);
  if (rc) return rc;
  uint64_t width = 0;
  if ((rc = gm_ks_level_size(s, level, &width))) return rc;
  if (!width) return 0;
  if (!offsets_dev || !child_words_dev) return fail(GM_EINVAL, "bad argument");
  GM_KS_LAUNCH_PLAIN(k_ks_reduce, ks_grid(s, width), s, s->d, s->tab, s->mask, s->lv, s->lcap, s->st, level,
                   offsets_dev, child_words_dev);
  HIPCHK(hipGetLastError());
  return ks_errors(s);
}

int gm_ks_end(gm_solver* s, gm_result* out) {
  int rc = ks_check(s, 0);
  if (rc) return rc;
  if (!out) return fail(GM_EINVAL, "null result");
  memset(out, 0, sizeof *out);
  const int T = s->d.max_levels;
  hipLaunchKernelGGL(k_root_word, dim3(1), dim3(64), 0, s->stream, s->tab, s->mask, s->d.root, s->st);
  HIPCHK(hipGetLastError());
  std::vector<unsigned char> host(devstate_bytes(T));
  HIPCHK(hipMemcpyAsync(host.data(), s->st, host.size(), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  const DevState* hs = (const DevState*)host.data();
  out->positions = hs->cursor_front + hs->cursor_back;
  out->edges = hs->edges;
  out->primitives = hs->prims;
  out->max_level_width = (uint32_t)hs->max_width;
  uint32_t lv = 0;
  for (int L = 0; L < T; L++) {
    const LevelSeg& g = hs->seg[L];
    if ((g.fe - g.fb) + (g.c2hi - g.c2lo) > 0) lv++;
  }
  out->levels = lv;
  out->root_word = hs->root_word;  // NO_WORD on every rank but the root's owner
  if (hs->root_word != NO_WORD) {
    out->root_value = (int32_t)(hs->root_word & 3u);
    out->root_remoteness = hs->root_word >> 2;
  }
  if (hs->err) {
    bool full = hs->err & (ERR_TABLE_FULL | ERR_LEVELS_FULL);
    return fail(full ? GM_EFULL : GM_ECORRUPT, "shard %d/%d:%s", s->rank, s->world, err_text(hs->err).c_str());
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Explicit-graph retrograde for game files without a device descriptor
// (SURVEY §8f row 3): the host enumerates the positions with the module's
// own gen_moves/do_move/primitive (gamesmanmpi_amd/generic.py) and hands
// over a CSR graph; the device resolves it in rounds.  A round resolves
// every position whose children are all resolved (any order of positions
// inside a round is fine: a word, once written, is final), so the number of
// rounds is the height of the DAG.  No progress with the root unresolved
// means a cycle (the reference's job loop would never finish either).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_graph_round(const uint8_t* prim, const uint64_t* offsets,
                                                     const uint32_t* children, uint64_t n, uint32_t* words,
                                                     DevState* st) {
  u64 done = 0, edges = 0, prims = 0;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    if (words[i] != NO_WORD) continue;
    const int p = prim[i];
    uint32_t word;
    if (p != UNDECIDED) {
      word = make_word(p, 0);  // process.py:120-123: primitive, remoteness 0
      prims++;
    } else {
      const u64 a = offsets[i], b = offsets[i + 1];
      bool ready = true, any_loss = false, any_tie = false, any_draw = false;
      uint32_t min_loss = 0xFFFFFFFFu, max_all = 0;
      for (u64 j = a; j < b && ready; j++) {
        const uint32_t w = __hip_atomic_load(&words[children[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == NO_WORD) {
          ready = false;
          break;
        }
        const uint32_t v = w & 3u, r = w >> 2;
        if (v == LOSS) { any_loss = true; min_loss = min(min_loss, r); }
        any_tie |= (v == TIE);
        any_draw |= (v == DRAW);
        max_all = max(max_all, r);
      }
      if (!ready) continue;
      if (a == b) {  // no moves but not primitive: the reference's job never resolves
        atomicOr(&st->err, ERR_NO_MOVES);
        continue;
      }
      // reference-canonical _res_red / _remote_red
      if (any_loss) word = make_word(WIN, min_loss + 1);
      else word = make_word(any_tie ? TIE : any_draw ? DRAW : LOSS, max_all + 1);
      edges += b - a;
    }
    __hip_atomic_store(&words[i], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    done++;
  }
  block_add(&st->cursor_front, done);
  block_add(&st->edges, edges);
  block_add(&st->prims, prims);
}

int gm_graph_solve(const uint8_t* prim_dev, const uint64_t* offsets_dev, const uint32_t* children_dev, uint64_t n,
                   uint64_t root, uint32_t* words_dev, void* scratch_dev, void* stream, gm_result* out) {
  if (!out || !n || root >= n || !prim_dev || !offsets_dev || !words_dev || !scratch_dev)
    return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GM_ENOGPU, "no HIP device");
  hipStream_t s = (hipStream_t)stream;
  DevState* st = (DevState*)scratch_dev;
  const int grid = (int)std::max<u64>(1, std::min<u64>((n + kBlock - 1) / kBlock, (u64)launch_grid()));
  auto t0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemsetAsync(words_dev, 0xFF, n * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(st, 0, sizeof(DevState), s));
  u64 resolved = 0, rounds = 0;
  uint32_t root_word = NO_WORD;
  for (;;) {
    hipLaunchKernelGGL(k_graph_round, dim3(grid), dim3(kBlock), 0, s, prim_dev, offsets_dev, children_dev, n,
                       words_dev, st);
    HIPCHK(hipGetLastError());
    rounds++;
    u64 now = 0;
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&now, &st->cursor_front, sizeof now, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, &st->err, sizeof err, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err) return fail(GM_ECORRUPT, "graph solve:%s", err_text(err).c_str());
    if (now == resolved) break;  // no progress: done, or a cycle
    resolved = now;
    if (resolved == n) break;
  }
  HIPCHK(hipMemcpyAsync(&root_word, words_dev + root, sizeof root_word, hipMemcpyDeviceToHost, s));
  DevState hs;
  HIPCHK(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  out->positions = hs.cursor_front;
  out->edges = hs.edges;
  out->primitives = hs.prims;
  out->levels = (uint32_t)rounds;
  out->n_resolve_launches = rounds;
  out->root_word = root_word;
  if (resolved != n)
    return fail(GM_ECORRUPT, "%llu of %llu positions never resolve (cycle)", (unsigned long long)(n - resolved),
                (unsigned long long)n);
  out->root_value = (int32_t)(root_word & 3u);
  out->root_remoteness = root_word >> 2;
  return 0;
}

#include "gm_graph_loopy.h"
