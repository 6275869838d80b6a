// Explicit-graph retrograde for game files whose positions repeat
// (gm_graph_solve_loopy; included by gm_solver.hip after
// gm_graph_solve).  A graph with cycles leaves gm_graph_solve's rule -- resolve
// a position once all its children are resolved -- with positions it never
// reaches; here they get a word too, in four phases:
//
//   A  founded positions: gm_graph_solve's own round loop (k_graph_round) to
//      its fixpoint.  No cycle is reachable from a founded position; its word
//      is the reference reducer's.  A graph without cycles ends here, with the
//      launches and the words of gm_graph_solve.
//   B  WIN / LOSS attractor over the positions A left open: WIN if some child
//      is LOSS (1 + the least remoteness of its LOSS children), LOSS if every
//      child is WIN (1 + the largest child remoteness).
//   C  TIE over what B left open: TIE if some child is TIE (1 + the least
//      remoteness of its TIE children).
//   D  whatever is still open is DRAW, remoteness 0.
//
// B and C run rounds k = 1, 2, .. synchronous in remoteness: in round k a
// reader ignores every child word of remoteness >= k, and a word written in
// round k carries remoteness k.  So a reader of round k never uses a word
// written in round k, whether it sees the store or not -- no double buffer,
// and no thread waits on another thread's store: every dependency is a launch
// boundary or a counter the host reads.  "First LOSS child seen" would not be
// "least remoteness": a founded LOSS child of remoteness 4 exists before an
// attractor LOSS child of remoteness 2 does; the filter shows the parent the
// child of remoteness 2 first, in round 3.
//
// A round that resolves nothing leaves the words as they were, so the next
// round that can differ is the one that first shows an ignored word: the
// round reports the least ignored remoteness r >= k it met on a child that
// could matter (LoopyState::next) and the host goes on with k = r + 1; with
// nothing ignored the phase is at its fixpoint.  The rounds of B and C walk a
// compacted list of the open positions (k_loopy_compact), compacted again
// whenever half of it has resolved.
//
// Scratch (GM_GRAPH_LOOPY_SCRATCH_BYTES(n) = 4096 + 8 n): DevState at 0,
// LoopyState at 2048, two lists of n position ids from 4096.
#pragma once

struct LoopyState {
  u64 resolved;      // positions resolved by phases B and C so far
  u64 cursor;        // k_loopy_compact: entries appended
  uint32_t next[2];  // least ignored remoteness of a round, by launch parity
};
constexpr size_t kLoopyStateOffset = 2048, kLoopyListOffset = 4096;
static_assert(sizeof(DevState) <= kLoopyStateOffset, "DevState overlaps LoopyState");
static_assert(kLoopyStateOffset + sizeof(LoopyState) <= kLoopyListOffset, "LoopyState overlaps the lists");
constexpr uint32_t kLoopyNone = 0xFFFFFFFFu;

// dst[0 .. *cursor) = the positions of src[0 .. nsrc) (src == nullptr: the
// positions 0 .. nsrc) without a word, in no particular order.  One atomic
// per wave; every lane of a wave takes the same number of steps.
__global__ __launch_bounds__(256) void k_loopy_compact(const uint32_t* src, u64 nsrc, const uint32_t* words,
                                                       uint32_t* dst, u64* cursor) {
  const int lane = __lane_id();
  for (u64 base = (u64)blockIdx.x * blockDim.x; base < nsrc; base += (u64)gridDim.x * blockDim.x) {
    const u64 j = base + threadIdx.x;
    uint32_t i = 0;
    bool open = false;
    if (j < nsrc) {
      i = src ? src[j] : (uint32_t)j;
      open = words[i] == NO_WORD;
    }
    const u64 mask = __ballot(open);
    if (!mask) continue;
    u64 at = 0;
    if (lane == 0) at = atomicAdd(cursor, (u64)__popcll(mask));
    at = __shfl(at, 0);
    if (open) dst[at + __popcll(mask & ((1ull << lane) - 1))] = i;
  }
}

// One round of phase B (TIES = false) or C (TIES = true) over the open list.
template <bool TIES>
__global__ __launch_bounds__(256) void k_loopy_round(const uint32_t* list, u64 m, const uint64_t* offsets,
                                                     const uint32_t* children, uint32_t* words, uint32_t k, int slot,
                                                     LoopyState* ls, DevState* st) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ls->next[slot ^ 1] = kLoopyNone;  // the next launch's; nobody reads it now
  u64 done = 0, edges = 0;
  uint32_t next = kLoopyNone;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (u64)gridDim.x * blockDim.x) {
    const uint32_t i = list[t];
    if (words[i] != NO_WORD) continue;
    const u64 a = offsets[i], b = offsets[i + 1];
    u64 wins = 0;
    uint32_t least = kLoopyNone, most = 0;  // least: over the usable LOSS (TIES: TIE) children; most: over the WIN
    for (u64 j = a; j < b; j++) {
      const uint32_t w = __hip_atomic_load(&words[children[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == NO_WORD) continue;
      const uint32_t v = w & 3u, r = w >> 2;
      if (TIES ? v != TIE : v > LOSS) continue;  // no part in this phase
      if (r >= k) {  // not before round r + 1
        next = min(next, r);
        continue;
      }
      if (TIES || v == LOSS) {
        least = min(least, r);
      } else {
        wins++;
        most = max(most, r);
      }
    }
    uint32_t word;
    if (least != kLoopyNone) word = make_word(TIES ? TIE : WIN, least + 1);
    else if (!TIES && wins == b - a) word = make_word(LOSS, most + 1);
    else continue;
    __hip_atomic_store(&words[i], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    done++;
    edges += b - a;
  }
  for (int o = 32; o > 0; o >>= 1) next = min(next, (uint32_t)__shfl_xor((int)next, o));
  if (__lane_id() == 0 && next != kLoopyNone) atomicMin(&ls->next[slot], next);
  block_add(&ls->resolved, done);
  block_add(&st->edges, edges);
}

// Phase D: every listed position still without a word is DRAW in 0.
__global__ __launch_bounds__(256) void k_loopy_draw(const uint32_t* list, u64 m, const uint64_t* offsets,
                                                    uint32_t* words, DevState* st) {
  u64 edges = 0;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (u64)gridDim.x * blockDim.x) {
    const uint32_t i = list[t];
    if (words[i] != NO_WORD) continue;
    words[i] = make_word(DRAW, 0);
    edges += offsets[i + 1] - offsets[i];
  }
  block_add(&st->edges, edges);
}

namespace {
struct LoopyRun {
  hipStream_t s;
  const uint64_t* offsets;
  const uint32_t* children;
  uint32_t* words;
  DevState* st;
  LoopyState* ls;
  uint32_t* list[2];
  int cur = 0;     // list[cur] holds the open positions
  u64 len = 0;     // its length
  u64 open = 0;    // of them still without a word
  u64 seen = 0;    // LoopyState::resolved at the last read
  u64 rounds = 0;  // launches of k_graph_round and k_loopy_round
  u64 cap = 0;
  int launches = 0;  // parity of the next k_loopy_round
};

static int loopy_grid(u64 m) { return (int)std::max<u64>(1, std::min<u64>((m + kBlock - 1) / kBlock, (u64)launch_grid())); }

// list[cur ^ 1] = the open positions of src (list[cur], or all n positions)
static int loopy_compact(LoopyRun& r, const uint32_t* src, u64 nsrc) {
  HIPCHK(hipMemsetAsync(&r.ls->cursor, 0, sizeof(u64), r.s));
  hipLaunchKernelGGL(k_loopy_compact, dim3(loopy_grid(nsrc)), dim3(kBlock), 0, r.s, src, nsrc, r.words,
                     r.list[r.cur ^ 1], &r.ls->cursor);
  HIPCHK(hipGetLastError());
  u64 got = 0;
  HIPCHK(hipMemcpyAsync(&got, &r.ls->cursor, sizeof got, hipMemcpyDeviceToHost, r.s));
  HIPCHK(hipStreamSynchronize(r.s));
  if (got != r.open) return fail(GM_ECORRUPT, "loopy graph solve: %llu open positions listed, %llu expected",
                                 (unsigned long long)got, (unsigned long long)r.open);
  r.cur ^= 1;
  r.len = got;
  return 0;
}

// Phase B or C to its fixpoint; *count = positions it resolved.
template <bool TIES>
static int loopy_phase(LoopyRun& r, u64* count) {
  *count = 0;
  uint32_t k = 1;
  while (r.open) {
    if (r.rounds >= r.cap) return fail(GM_ECORRUPT, "loopy graph solve: more than %llu rounds", (unsigned long long)r.cap);
    const int slot = r.launches++ & 1;
    hipLaunchKernelGGL(k_loopy_round<TIES>, dim3(loopy_grid(r.len)), dim3(kBlock), 0, r.s, r.list[r.cur], r.len,
                       r.offsets, r.children, r.words, k, slot, r.ls, r.st);
    HIPCHK(hipGetLastError());
    r.rounds++;
    LoopyState h;
    HIPCHK(hipMemcpyAsync(&h, r.ls, sizeof h, hipMemcpyDeviceToHost, r.s));
    HIPCHK(hipStreamSynchronize(r.s));
    const u64 now = h.resolved - r.seen;
    r.seen = h.resolved;
    *count += now;
    r.open -= now;
    if (now) k++;  // words of remoteness k exist now
    else if (h.next[slot] == kLoopyNone) break;  // nothing resolved, nothing ignored: the fixpoint
    else k = h.next[slot] + 1;  // the rounds in between would see what this one saw
    if (r.open && r.len >= 1024 && r.open <= r.len / 2) {
      int rc = loopy_compact(r, r.list[r.cur], r.len);
      if (rc) return rc;
    }
  }
  return 0;
}
}  // namespace

int gm_graph_solve_loopy(const uint8_t* prim_dev, const uint64_t* offsets_dev, const uint32_t* children_dev, uint64_t n,
                         uint64_t root, uint32_t* words_dev, void* scratch_dev, void* stream, gm_result* out,
                         uint64_t counts[4]) {
  if (!out || !n || root >= n || n > 0xFFFFFFFFull || !prim_dev || !offsets_dev || !words_dev || !scratch_dev)
    return fail(GM_EINVAL, "bad argument");
  memset(out, 0, sizeof *out);
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GM_ENOGPU, "no HIP device");
  LoopyRun r;
  r.s = (hipStream_t)stream;
  r.offsets = offsets_dev;
  r.children = children_dev;
  r.words = words_dev;
  r.st = (DevState*)scratch_dev;
  r.ls = (LoopyState*)((char*)scratch_dev + kLoopyStateOffset);
  r.list[0] = (uint32_t*)((char*)scratch_dev + kLoopyListOffset);
  r.list[1] = r.list[0] + n;
  r.cap = 2 * n + 8;
  hipStream_t s = r.s;
  DevState* st = r.st;
  const int grid = loopy_grid(n);
  auto t0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemsetAsync(words_dev, 0xFF, n * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(st, 0, sizeof(DevState), s));
  // phase A: gm_graph_solve's loop, which a cycle ends early instead of failing
  u64 founded = 0;
  for (;;) {
    hipLaunchKernelGGL(k_graph_round, dim3(grid), dim3(kBlock), 0, s, prim_dev, offsets_dev, children_dev, n,
                       words_dev, st);
    HIPCHK(hipGetLastError());
    r.rounds++;
    u64 now = 0;
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&now, &st->cursor_front, sizeof now, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, &st->err, sizeof err, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err) return fail(GM_ECORRUPT, "graph solve:%s", err_text(err).c_str());
    if (now == founded) break;
    founded = now;
    if (founded == n) break;
  }
  u64 c[4] = {founded, 0, 0, n - founded};
  if (founded != n) {
    HIPCHK(hipMemsetAsync(r.ls, 0, sizeof(LoopyState), s));
    HIPCHK(hipMemsetAsync(r.ls->next, 0xFF, sizeof r.ls->next, s));
    r.open = n - founded;
    r.cur = 1;  // loopy_compact fills the other list: list[0]
    int rc = loopy_compact(r, nullptr, n);
    if (!rc) rc = loopy_phase<false>(r, &c[1]);
    if (!rc) rc = loopy_phase<true>(r, &c[2]);
    if (rc) return rc;
    c[3] = r.open;
    if (r.open) {
      hipLaunchKernelGGL(k_loopy_draw, dim3(loopy_grid(r.len)), dim3(kBlock), 0, s, r.list[r.cur], r.len, offsets_dev,
                         words_dev, st);
      HIPCHK(hipGetLastError());
    }
  }
  uint32_t root_word = NO_WORD;
  HIPCHK(hipMemcpyAsync(&root_word, words_dev + root, sizeof root_word, hipMemcpyDeviceToHost, s));
  DevState hs;
  HIPCHK(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  out->positions = n;
  out->edges = hs.edges;
  out->primitives = hs.prims;
  out->levels = (uint32_t)r.rounds;
  out->n_resolve_launches = r.rounds;
  out->root_word = root_word;
  out->root_value = (int32_t)(root_word & 3u);
  out->root_remoteness = root_word >> 2;
  if (counts) memcpy(counts, c, sizeof c);
  return 0;
}
