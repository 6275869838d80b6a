// gm_table_file.h -- a saved tablebase opened on the device
// (gm_table_check / gm_solver_open_table): the bytes of solution.gmtb
//  or solution.gmtk (7f) in HBM as one more layout,
// GM_MODE_FILE, behind the three views of gm_table.h.  The image IS the file:
// keys are not expanded, words are not widened, the footprint is the file's
// size.  DESIGN.md section 7j.
//
// Reference path replaced: reading a saved solution back one key at a time
// from the resolved / remote shelves (src/cache_dict.py:62-79).
//
//   gmtb  TbWords<WB>  key -> index (the GM_HD bodies gm_tb_index runs:
//                      tb_sum_index, rk_slot_of) -> bit test -> rank = the
//                      block's count + popcounts of the block's earlier
//                      bitmap words and the partial word -> one word load
//         TbEnum       one 64-index bitmap word per item, place: the rank
//         TbPairs<WB>  the word at that rank
//   gmtk  TkWords      any_canon -> mix64 -> two directory entries -> lower
//                      bound over the bucket's cut keys -> the word there
//         TkEnum       item i = the i-th stored key, place: i
//         TkPairs      the word at i
// A gmtb holds games whose layouts do not canonise (sum games; toot without
// board symmetry: tb_space refuses the others), so TbWords does not either;
// TkWords canonises with the descriptor's flags as hashed_word / bk_word do.
//
// There are no storage-order census / export kernels for this mode: the `how`
// argument of gm_solver_census / gm_solver_export / gm_solver_export_keyed is
// ignored, every call takes the generic path.
//
// Two sections.  The first (the views, the validation kernel templates) is
// included by gm_solver.hip inside its extern "C" block after every layout
// header, before gm_table.h.  The second (GM_TABLE_FILE_HOST defined: the
// host check and the open) is included at the end of the C-ABI, so that the
// kernels only it instantiates come last in the code object.
#ifndef GM_TABLE_FILE_HOST
extern "C++" {

// ---------------------------------------------------------------------------
// the file formats (gamesmanmpi_amd/db.py states them)
// ---------------------------------------------------------------------------
constexpr u64 kTfHeader = 64;
constexpr uint32_t kTfVersion = 1;
static const char kTbMagic[9] = "GMTBASE1";
static const char kTkMagic[9] = "GMTBKEY1";

// sum games: index = key, for the keys of the rank space (gm_tb_index)
GM_HD u64 tb_sum_index(u64 total, u64 key) { return key < total ? key : GM_NO_INDEX; }
// bucket of a key in a keyed tablebase
__device__ __forceinline__ u64 tk_bucket(u64 key, uint32_t b) { return b ? mix64(key) >> (64u - b) : 0ull; }

struct TbGeom {
  const u64* bits;       // [space / 64]
  const u64* counts;     // [space / 512 + 1]
  const uint8_t* words;  // [positions * WB], 8-byte aligned
  u64 space, positions;
  u64 total;             // sum games: keys of the rank space
  bool toot;
  RankGeom g;            // toot: C, H, A, T, stride, nslots; base and lvph in the open's scratch
  const u64* lvt;        // toot: RankEnum's level tables (gm_table.h)
};
struct TkGeom {
  const u64* dir;        // [2^b + 1]
  const uint8_t* keys;   // [positions * kb]
  const uint8_t* words;  // [positions * wb], any alignment
  u64 positions;
  uint32_t kb, wb, b;
};

template <int WB>
__device__ __forceinline__ uint32_t tb_word_at(const TbGeom& t, u64 rank) {
  if (rank >= t.positions) return NO_WORD;
  if (WB == 1) return t.words[rank];
  if (WB == 2) return reinterpret_cast<const uint16_t*>(t.words)[rank];
  return reinterpret_cast<const uint32_t*>(t.words)[rank];
}
// reached indexes below index wi * 64 + bit (m: bitmap word wi)
__device__ __forceinline__ u64 tb_rank(const TbGeom& t, u64 wi, u64 m, uint32_t bit) {
  u64 r = t.counts[wi >> 3];
  for (u64 j = wi & ~7ull; j < wi; j++) r += (u64)__builtin_popcountll(t.bits[j]);
  return r + (u64)__builtin_popcountll(m & ((1ull << bit) - 1ull));
}
// is `idx` (< space) the index of a position?  (gm_export.h ExportIndex::key's test)
__device__ __forceinline__ bool tb_index_ok(const TbGeom& t, u64 idx) {
  if (!t.toot) return idx < t.total;
  const u64* lvstart = t.lvt;
  const u64* lvoff = t.lvt + t.g.T + 1;
  uint32_t L = 0;
  while (L + 1 < t.g.T && lvstart[L + 1] <= idx) L++;
  const u64 i = idx - lvstart[L];
  if ((i >> (L + 3)) >= lvoff[L + 1] - lvoff[L]) return false;  // the level's padding
  const uint32_t a = (uint32_t)((i >> L) & 7u), pat = (uint32_t)(i & ((1ull << L) - 1));
  return rk_valid(rk_hands(L, (uint32_t)__builtin_popcount(pat), a));
}

__device__ __forceinline__ u64 tk_key_at(const TkGeom& t, u64 i) {
  const uint8_t* p = t.keys + i * t.kb;
  u64 k = 0;
  for (uint32_t j = 0; j < t.kb; j++) k |= (u64)p[j] << (8u * j);
  return k;
}
__device__ __forceinline__ uint32_t tk_word_at(const TkGeom& t, u64 i) {
  if (i >= t.positions) return NO_WORD;
  const uint8_t* p = t.words + i * t.wb;
  uint32_t w = 0;
  for (uint32_t j = 0; j < t.wb; j++) w |= (uint32_t)p[j] << (8u * j);
  return w;
}

// ---------------------------------------------------------------------------
// word of key
// ---------------------------------------------------------------------------
template <int WB>
struct TbWords {
  TbGeom t;
  __device__ __forceinline__ uint32_t operator()(const Desc&, u64 key) const {
    u64 idx;
    if (t.toot) {
      uint32_t L;
      if (!rk_slot_of(t.g, key, &idx, &L)) return NO_WORD;
    } else {
      idx = tb_sum_index(t.total, key);
    }
    if (idx >= t.space) return NO_WORD;  // (GM_NO_INDEX too)
    const u64 wi = idx >> 6, m = t.bits[wi];
    const uint32_t bit = (uint32_t)idx & 63u;
    if (!((m >> bit) & 1ull)) return NO_WORD;
    return tb_word_at<WB>(t, tb_rank(t, wi, m, bit));
  }
};
struct TkWords {
  TkGeom t;
  __device__ __forceinline__ uint32_t operator()(const Desc& d, u64 key0) const {
    const u64 key = any_canon(d, key0);  // symmetry hooks: the orbit's representative
    if (t.kb < 8 && (key >> (8u * t.kb))) return NO_WORD;  // a bit above the stored bytes
    const u64 h = tk_bucket(key, t.b);
    u64 lo = t.dir[h];
    const u64 end = min(t.dir[h + 1], t.positions);
    u64 hi = end;
    while (lo < hi) {  // lower bound of key in [lo, hi)
      const u64 mid = (lo + hi) >> 1;
      if (tk_key_at(t, mid) < key) lo = mid + 1;
      else hi = mid;
    }
    return lo < end && tk_key_at(t, lo) == key ? tk_word_at(t, lo) : NO_WORD;
  }
};

// ---------------------------------------------------------------------------
// position enumerators and pair sources (gm_table.h's contract; the adaptors
// visit_keys / visit_pairs are declared there, after this header)
// ---------------------------------------------------------------------------
template <class EN, class F>
__device__ __forceinline__ void visit_keys(const EN& en, const Desc& d, u64 i, F&& f);
template <class PS, class F>
__device__ __forceinline__ void visit_pairs(const PS& ps, const Desc& d, u64 i, F&& f);

struct TbEnum {  // one 64-index word of the bitmap per item; place: the rank
  static constexpr bool kOnePerItem = false;
  TbGeom t;
  __device__ __forceinline__ u64 items() const { return t.space / 64; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 wi, N&& n, F&& f) const {
    u64 m = t.bits[wi];
    if (!m) return;
    const u64* lvstart = t.lvt;
    const u64* lvoff = t.lvt + t.g.T + 1;
    const u64 s0 = wi << 6;
    uint32_t L = 0;  // (toot levels start 512-aligned: a word belongs to one level)
    if (t.toot)
      while (L + 1 < t.g.T && lvstart[L + 1] <= s0) L++;
    n((uint32_t)__builtin_popcountll(m));
    u64 rank = tb_rank(t, wi, m, 0);
    for (; m; m &= m - 1, rank++) {
      const u64 idx = s0 + (u64)__builtin_ctzll(m);
      f(t.toot ? rk_slot_key(t.g, lvstart, lvoff, L, idx) : idx, rank);
    }
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
template <int WB>
struct TbPairs : TbEnum {
  __device__ __forceinline__ uint32_t word(u64, u64 rank) const { return tb_word_at<WB>(t, rank); }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

struct TkEnum {  // the stored keys in file order; place: i
  static constexpr bool kOnePerItem = true;
  TkGeom t;
  __device__ __forceinline__ u64 items() const { return t.positions; }
  template <class N, class F>
  __device__ __forceinline__ void each(const Desc&, u64 i, N&& n, F&& f) const {
    n(1u);
    f(tk_key_at(t, i), i);
  }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_keys(*this, d, i, f);
  }
};
struct TkPairs : TkEnum {  // the stored keys are their orbits' representatives: no any_canon
  __device__ __forceinline__ uint32_t word(u64, u64 i) const { return tk_word_at(t, i); }
  template <class F>
  __device__ __forceinline__ void visit(const Desc& d, u64 i, F&& f) const {
    visit_pairs(*this, d, i, f);
  }
};

// ---------------------------------------------------------------------------
// validation: every range the views follow, checked once at open
// ---------------------------------------------------------------------------
// bad[0]: the first block / bucket whose counts / directory entries are wrong,
// bad[1]: the first whose bitmap / keys are; ~0: none.  Templates (over the
// image's geometry type) so that they are emitted where the open instantiates
// them, after every other kernel.
//
// gmtb, one thread per 512-index block: counts[0] = 0, counts never decrease,
// each step = the popcount of the block's eight bitmap words, the last count =
// positions; every set bit is the index of a position (so TbEnum's key of an
// index reads inside the level tables).
template <class TB>
__global__ __launch_bounds__(256) void k_tb_validate(TB t, u64* __restrict__ bad) {
  const u64 nblk = t.space / GM_TB_BLOCK;
  for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += (u64)gridDim.x * blockDim.x) {
    const u64 c0 = t.counts[b], c1 = t.counts[b + 1];
    u64 pop = 0;
    bool keys_ok = true;
    for (u64 j = 0; j < 8; j++) {
      u64 m = t.bits[b * 8 + j];
      pop += (u64)__builtin_popcountll(m);
      for (; m; m &= m - 1) keys_ok = keys_ok && tb_index_ok(t, ((b * 8 + j) << 6) + (u64)__builtin_ctzll(m));
    }
    if (c1 < c0 || c1 - c0 != pop || c1 > t.positions || (b == 0 && c0 != 0) || (b == nblk - 1 && c1 != t.positions))
      atomicMin(&bad[0], b);
    if (!keys_ok) atomicMin(&bad[1], b);
  }
}
// gmtk, one wave per bucket: dir[0] = 0, the directory never decreases and
// ends at positions; the bucket's keys ascend strictly.  The keys are read
// only inside a range that passed the directory test.
template <class TK>
__global__ __launch_bounds__(256) void k_tk_validate(TK t, u64* __restrict__ bad) {
  const u64 nb = 1ull << t.b;
  const uint32_t lane = __lane_id();
  const u64 nwaves = (u64)gridDim.x * (blockDim.x >> 6);
  for (u64 h = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); h < nb; h += nwaves) {
    const u64 o0 = t.dir[h], o1 = t.dir[h + 1];
    if (o1 < o0 || o1 > t.positions || (h == 0 && o0 != 0) || (h == nb - 1 && o1 != t.positions)) {
      if (lane == 0) atomicMin(&bad[0], h);
      continue;
    }
    bool ok = true;
    for (u64 i = o0 + lane; i + 1 < o1; i += 64) ok = ok && tk_key_at(t, i) < tk_key_at(t, i + 1);
    if (!ok) atomicMin(&bad[1], h);
  }
}

}  // extern "C++"
#else  // GM_TABLE_FILE_HOST
extern "C++" {

// ---------------------------------------------------------------------------
// host: a header against a byte count (db.Tablebase / db.KeyedTablebase's tests)
// ---------------------------------------------------------------------------
struct TfInfo {
  uint32_t format;  // 1 gmtb, 2 gmtk
  uint32_t wb, kb, b;
  u64 positions, space;
  u64 off0, off1, words_off;  // bitmap | directory, counts | keys, words
  u64 index_bytes;            // device bytes of the index tables (toot gmtb), after the solver's state
  u64 base_off, lvt_off, lvph_off;  // inside the index tables
};
static u64 tf_rd64(const uint8_t* p) {
  u64 v;
  memcpy(&v, p, 8);
  return v;
}
static uint32_t tf_rd32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

static int table_check(const Desc* d, const uint8_t* head, u64 head_bytes, u64 file_bytes, TfInfo* o) {
  memset(o, 0, sizeof *o);
  if (head_bytes < kTfHeader) return fail(GM_EINVAL, "gm_table_check: %llu header bytes, a tablebase has %llu",
                                          (unsigned long long)head_bytes, (unsigned long long)kTfHeader);
  const bool tb = !memcmp(head, kTbMagic, 8), tk = !memcmp(head, kTkMagic, 8);
  if (!tb && !tk) return fail(GM_EINVAL, "no tablebase (bad magic)");
  const uint32_t version = tf_rd32(head + 8);
  if (version != kTfVersion) return fail(GM_EINVAL, "tablebase version %u, this reader knows %u", version, kTfVersion);
  o->wb = tf_rd32(head + 12);
  if (o->wb != 1 && o->wb != 2 && o->wb != 4) return fail(GM_EINVAL, "bad header (word bytes %u)", o->wb);
  u64 total;
  if (tb) {
    o->format = 1;
    o->space = tf_rd64(head + 16);
    o->positions = tf_rd64(head + 24);
    o->off0 = tf_rd64(head + 32);
    o->off1 = tf_rd64(head + 40);
    o->words_off = tf_rd64(head + 48);
    total = tf_rd64(head + 56);
    if (o->space % GM_TB_BLOCK || o->space > (1ull << 56) || o->positions > o->space)
      return fail(GM_EINVAL, "bad header (index space %llu, %llu positions)", (unsigned long long)o->space,
                  (unsigned long long)o->positions);
    const u64 counts_off = kTfHeader + o->space / 8, words_off = counts_off + 8 * (o->space / GM_TB_BLOCK + 1);
    if (o->off0 != kTfHeader || o->off1 != counts_off || o->words_off != words_off ||
        total != words_off + o->positions * o->wb)
      return fail(GM_EINVAL, "section offsets do not match the header's sizes");
  } else {
    o->format = 2;
    o->kb = tf_rd32(head + 16);
    o->b = tf_rd32(head + 20);
    o->positions = tf_rd64(head + 24);
    o->off0 = tf_rd64(head + 32);
    o->off1 = tf_rd64(head + 40);
    o->words_off = tf_rd64(head + 48);
    total = tf_rd64(head + 56);
    if (o->kb < 1 || o->kb > 8 || o->b > 32 || o->positions > (1ull << 56))
      return fail(GM_EINVAL, "bad header (key bytes %u / bucket bits %u / %llu positions)", o->kb, o->b,
                  (unsigned long long)o->positions);
    const u64 keys_off = kTfHeader + 8 * ((1ull << o->b) + 1), words_off = keys_off + o->positions * o->kb;
    if (o->off0 != kTfHeader || o->off1 != keys_off || o->words_off != words_off ||
        total != words_off + o->positions * o->wb)
      return fail(GM_EINVAL, "section offsets do not match the header's sizes");
  }
  if (file_bytes != total)
    return fail(GM_EINVAL, "%llu bytes, the header says %llu (truncated?)", (unsigned long long)file_bytes,
                (unsigned long long)total);
  if (tb) {
    u64 space = 0;
    RankShape rs;
    const int rc = tb_space(d, &space, &rs);
    if (rc) return rc;
    if (space != o->space)
      return fail(GM_EINVAL, "index space %llu, the game has %llu", (unsigned long long)o->space,
                  (unsigned long long)space);
    if (d->kind == K_TOOT) {  // base[hvcode], the level tables, the packed heights
      o->base_off = 0;
      o->lvt_off = o->base_off + rs.base.size() * sizeof(u64);
      o->lvph_off = o->lvt_off + 2 * ((u64)rs.g.T + 1) * sizeof(u64);
      o->index_bytes = (o->lvph_off + rs.lvph.size() * sizeof(uint32_t) + 255) / 256 * 256;
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// host: the open
// ---------------------------------------------------------------------------
static int table_open(const Desc* d, const void* image_dev, u64 bytes, void* scratch, u64 scratch_bytes, void* stream,
                      gm_solver** out) {
  if (bytes < kTfHeader) return fail(GM_EINVAL, "gm_solver_open_table: %llu bytes hold no header", (unsigned long long)bytes);
  if (((uintptr_t)image_dev | (uintptr_t)scratch) & 255u)
    return fail(GM_EINVAL, "gm_solver_open_table: the image and the scratch buffer are 256-byte aligned");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GM_ENOGPU, "no HIP device");
  uint8_t head[kTfHeader];
  HIPCHK(hipMemcpy(head, image_dev, sizeof head, hipMemcpyDeviceToHost));
  TfInfo fi;
  int rc = table_check(d, head, sizeof head, bytes, &fi);
  if (rc) return rc;
  const u64 state = (scratch_bytes_for(d->max_levels) + 255) / 256 * 256;
  if (scratch_bytes < state + fi.index_bytes)
    return fail(GM_EINVAL, "gm_solver_open_table: scratch of %llu bytes, the table needs %llu (gm_table_check)",
                (unsigned long long)scratch_bytes, (unsigned long long)(state + fi.index_bytes));
  std::unique_ptr<gm_solver, void (*)(gm_solver*)> sp(new gm_solver(), gm_solver_destroy);
  gm_solver* s = sp.get();
  s->d = *d;
  s->mode = GM_MODE_FILE;
  s->rank = 0;
  s->world = 1;
  s->comm = nullptr;
  s->words = nullptr;
  s->bits = nullptr;
  s->tab = nullptr;
  s->mask = 0;
  s->lv = nullptr;
  s->lcap = 0;
  s->nslots = 0;
  s->nblocks = 0;
  s->masks = nullptr;
  s->flags = 0;
  s->st = (DevState*)scratch;
  s->grid = launch_grid();
  if (stream) {
    s->stream = (hipStream_t)stream;
    s->own_stream = false;
  } else {
    s->own_stream = false;
    const hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(GM_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    s->own_stream = true;
  }
  const uint8_t* img = (const uint8_t*)image_dev;
  uint8_t* xtab = (uint8_t*)scratch + state;
  s->tf_format = fi.format;
  s->tf_wb = fi.wb;
  HIPCHK(hipMemsetAsync(s->st, 0, devstate_bytes(d->max_levels), s->stream));
  u64* bad = s->st->ck;  // (the checksum's accumulators: free until the first reader)
  HIPCHK(hipMemsetAsync(bad, 0xFF, 2 * sizeof(u64), s->stream));
  if (fi.format == 1) {
    s->tb = new TbGeom();
    TbGeom& t = *s->tb;
    t.bits = (const u64*)(img + fi.off0);
    t.counts = (const u64*)(img + fi.off1);
    t.words = img + fi.words_off;
    t.space = fi.space;
    t.positions = fi.positions;
    t.toot = d->kind == K_TOOT;
    if (!t.toot) {
      t.total = tb_sum_total(d);
    } else {
      RankShape rs;
      rc = rank_shape(d, &rs);
      if (rc) return rc;
      std::vector<u64> lvt(2 * ((size_t)rs.g.T + 1));
      for (uint32_t L = 0; L <= rs.g.T; L++) {
        lvt[L] = rs.lvstart[L];
        lvt[rs.g.T + 1 + L] = rs.lvoff[L];
      }
      HIPCHK(hipMemcpyAsync(xtab + fi.base_off, rs.base.data(), rs.base.size() * sizeof(u64), hipMemcpyHostToDevice,
                            s->stream));
      HIPCHK(hipMemcpyAsync(xtab + fi.lvt_off, lvt.data(), lvt.size() * sizeof(u64), hipMemcpyHostToDevice, s->stream));
      HIPCHK(hipMemcpyAsync(xtab + fi.lvph_off, rs.lvph.data(), rs.lvph.size() * sizeof(uint32_t),
                            hipMemcpyHostToDevice, s->stream));
      HIPCHK(hipStreamSynchronize(s->stream));  // (the host vectors end with this block)
      t.g = rs.g;  // (no table pointers but base and lvph: the index map reads nothing else)
      t.g.base = (const u64*)(xtab + fi.base_off);
      t.g.lvph = (const uint32_t*)(xtab + fi.lvph_off);
      t.lvt = (const u64*)(xtab + fi.lvt_off);
    }
    const u64 nblk = t.space / GM_TB_BLOCK;
    const int grid = (int)std::max<u64>(1, std::min<u64>((nblk + kBlock - 1) / kBlock, (u64)s->grid));
    hipLaunchKernelGGL(k_tb_validate<TbGeom>, dim3(grid), dim3(kBlock), 0, s->stream, t, bad);
  } else {
    s->tk = new TkGeom();
    TkGeom& t = *s->tk;
    t.dir = (const u64*)(img + fi.off0);
    t.keys = img + fi.off1;
    t.words = img + fi.words_off;
    t.positions = fi.positions;
    t.kb = fi.kb;
    t.wb = fi.wb;
    t.b = fi.b;
    const u64 nb = 1ull << t.b;
    const int grid = (int)std::max<u64>(1, std::min<u64>((nb + 3) / 4, (u64)s->grid));
    hipLaunchKernelGGL(k_tk_validate<TkGeom>, dim3(grid), dim3(kBlock), 0, s->stream, t, bad);
  }
  HIPCHK(hipGetLastError());
  u64 hb[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hb, bad, sizeof hb, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemsetAsync(bad, 0, sizeof hb, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (fi.format == 1 && (hb[0] != ~0ull || hb[1] != ~0ull)) {
    if (hb[0] != ~0ull)
      return fail(GM_ECORRUPT, "gm_solver_open_table: block %llu: the counts and the bitmap disagree (a step that is not "
                               "the popcount of the block's bitmap words, or an end that is not the position count)",
                  (unsigned long long)hb[0]);
    return fail(GM_ECORRUPT, "gm_solver_open_table: block %llu: a reached index is no position of the game",
                (unsigned long long)hb[1]);
  }
  if (fi.format == 2 && (hb[0] != ~0ull || hb[1] != ~0ull)) {
    if (hb[0] != ~0ull)  // (first: a wrong entry also moves the end of the bucket before it)
      return fail(GM_ECORRUPT, "gm_solver_open_table: bucket %llu: the directory decreases, or does not run from 0 to "
                               "the position count", (unsigned long long)hb[0]);
    return fail(GM_ECORRUPT, "gm_solver_open_table: bucket %llu: its keys do not ascend strictly",
                (unsigned long long)hb[1]);
  }
  s->solved = true;
  *out = sp.release();
  return 0;
}

}  // extern "C++"
#endif  // GM_TABLE_FILE_HOST
