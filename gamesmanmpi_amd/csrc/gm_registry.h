// gm_registry.h -- the game registry (host only): a reference module's name
// and parameter string -> the descriptor block the kernels take (gm_games.h),
// the table of boards whose reachable counts are known, and the bodies of
// gm_game_lookup / gm_game_info / gm_root (C linkage from their declarations
// in gamesman.h).  Included by gm_solver.hip after its error helpers.  One build function per game; the kinds' rules, lists
// and per-kind facts are in gm_games.h, their canonical bytes in gm_codec.h.

static std::mutex g_mu;
static std::vector<Desc> g_games;

static int kv(const char* params, const char* key, int dflt) {
  if (!params) return dflt;
  size_t kl = strlen(key);
  for (const char* p = params; (p = strstr(p, key)); p += kl) {
    if ((p == params || p[-1] == ',') && p[kl] == '=') return atoi(p + kl + 1);
  }
  return dflt;
}

// column 0 and, per direction (1,0) (0,1) (1,1) (1,-1), the cells that start
// a line of `span` cells lying wholly on the board (so that no shifted copy
// wraps a row) and the direction's step in cell index
static void desc_line_masks(Desc& d, int span) {
  for (int y = 0; y < d.H; y++) d.col0 |= 1ull << (d.L * y);
  const int dxs[4] = {1, 0, 1, 1}, dys[4] = {0, 1, 1, -1};
  for (int i = 0; i < 4; i++) {
    uint64_t m = 0;
    for (int x = 0; x < d.L; x++)
      for (int y = 0; y < d.H; y++) {
        int ex = x + (span - 1) * dxs[i], ey = y + (span - 1) * dys[i];
        if (ex >= 0 && ex < d.L && ey >= 0 && ey < d.H) m |= 1ull << (d.L * y + x);
      }
    d.tmask[i] = m;
    d.tstep[i] = dxs[i] + d.L * dys[i];
  }
}

static int desc_sum(const char* name, const char* params, Desc& d) {
  d.kind = K_SUM;
  if (name[0] == 'f') {
    d.variant = 1;
    int start = kv(params, "start", 4);  // four_to_one.py:7-8
    if (start < 0) return fail(GM_EINVAL, "four_to_one start must be >= 0");
    d.nheaps = 1;
    d.heap[0] = (uint32_t)start;
  } else {
    const char* p = params ? strstr(params, "heaps=") : nullptr;
    if (!p) return fail(GM_EINVAL, "sum_four_to_one needs heaps=h0:h1:...");
    p += 6;
    while (*p && *p != ',') {
      if (d.nheaps >= 16) return fail(GM_EINVAL, "at most 16 heaps");
      long h = strtol(p, nullptr, 10);
      if (h < 0 || h > (1L << 30)) return fail(GM_EINVAL, "bad heap %ld", h);
      d.heap[d.nheaps++] = (uint32_t)h;
      while (*p && *p != ':' && *p != ',') p++;
      if (*p == ':') p++;
    }
    if (d.nheaps == 0) return fail(GM_EINVAL, "no heaps");
  }
  unsigned __int128 stride = 1;
  d.pow2 = 1;
  for (int i = 0; i < d.nheaps; i++) {
    d.base[i] = d.heap[i] + 1;
    d.stride[i] = (uint64_t)stride;
    if (d.base[i] & (d.base[i] - 1)) d.pow2 = 0;
    int sh = 0;
    while ((1ull << sh) < (uint64_t)stride) sh++;
    d.shift[i] = (uint32_t)sh;
    d.root += (uint64_t)d.heap[i] * d.stride[i];
    d.root_sum += d.heap[i];
    stride *= d.base[i];
    if (stride > ((unsigned __int128)1 << 62)) return fail(GM_EINVAL, "state space exceeds 2^62");
  }
  if (d.root_sum >= (1u << 30) - 2) return fail(GM_EINVAL, "remoteness would exceed 30 bits");
  d.max_levels = (int)d.root_sum + 1;
  // dense layout (see gm_dense.h)
  d.W = 1;
  for (int i = 1; i < d.nheaps; i++) {
    d.pstride[i] = d.W;
    int sh = 0;
    while ((1ull << sh) < d.W) sh++;
    d.pshift[i] = (uint32_t)sh;
    d.W *= d.base[i];
  }
  d.wshift = -1;
  if ((d.W & (d.W - 1)) == 0) {
    int sh = 0;
    while ((1ull << sh) < d.W) sh++;
    d.wshift = sh;
  }
  d.dense_ok = 1;
  return 0;
}

static int desc_ttt(const char* name, const char*, Desc& d) {
  d.kind = K_TTT;
  d.variant = name[0] == 'm';
  d.max_levels = 10;
  return 0;
}

static int desc_toot(const char*, const char* params, Desc& d) {
  d.kind = K_TOOT;
  d.L = kv(params, "length", 6);  // toot_and_otto_bitstring.py:8
  d.H = kv(params, "height", 4);
  d.A = d.L * d.H;
  if (d.L < 1 || d.H < 1 || 2 * d.A + 13 > 64)
    return fail(GM_EINVAL, "toot board %dx%d does not fit a 64-bit key (area <= 25)", d.L, d.H);
  d.nbits = (2 * d.A + 17 + 7) / 8 * 8;
  d.full = (1ull << d.A) - 1;
  desc_line_masks(d, 4);  // word starts
  // initial_position (:36-44): hands 6,6,6,6; turn bit 0 (player 2 first)
  for (int j = 0; j < 4; j++) d.root |= 6ull << (2 * d.A + 3 * j);
  d.max_levels = d.A + 1;
  return 0;
}

static int desc_othello(const char*, const char* params, Desc& d) {
  d.kind = K_OTHELLO;
  d.L = kv(params, "length", 8);  // othello_bit_new.py:8
  d.H = kv(params, "height", 8);
  d.A = d.L * d.H;
  if (d.L != d.H)
    return fail(GM_EINVAL, "othello descriptor supports square boards only (reference flip bounds "
                           "are transposed for non-square boards, othello_bit_new.py:101,110)");
  if (d.L < 2 || 2 * d.A + 3 > 64)
    return fail(GM_EINVAL, "othello board %dx%d does not fit a 64-bit key (area <= 30)", d.L, d.H);
  d.nbits = (2 * d.A + 16 + 7) / 8 * 8;
  d.full = (1ull << d.A) - 1;
  // initial_position (:37-48) with the module's float coordinates
  // (length / 2 - 1): board index int(length*y + x)
  auto put = [&](double x, double y, int white) {
    int idx = (int)(d.L * y + x);
    d.root |= 1ull << (white ? idx : d.A + idx);
  };
  double hx = d.L / 2.0, hy = d.H / 2.0;
  put(hx - 1, hy - 1, 1);
  put(hx - 1, hy, 0);
  put(hx, hy - 1, 0);
  put(hx, hy, 1);
  // two incr_turn calls from 0 -> turn_count 2 (WHITE): bit 2A = 0
  d.max_levels = d.A + 3;
  d.sym = kv(params, "symmetry", 0) ? 1 : 0;  // player_flip orbits (symmetry_functions, :224-226)
  d.root = oth_canon(d, d.root);
  return 0;
}

static int desc_connect(const char*, const char* params, Desc& d) {
  d.kind = K_CONNECT;
  d.L = kv(params, "length", 5);  // games/connect_four.py
  d.H = kv(params, "height", 4);
  d.variant = kv(params, "connect", 4);
  if (d.L < 1 || d.H < 1 || d.L > 8 || (long)d.L * d.H > 30)
    return fail(GM_EINVAL, "connect four board %dx%d: at most 8 columns and 30 cells fit the key "
                           "(two planes of L*H bits; 7x6 is out of reach)", d.L, d.H);
  d.A = d.L * d.H;
  if (d.variant < 1 || d.variant > (d.L > d.H ? d.L : d.H))
    return fail(GM_EINVAL, "connect=%d: a line on a %dx%d board has 1..%d cells", d.variant, d.L, d.H,
                d.L > d.H ? d.L : d.H);
  d.full = (1ull << d.A) - 1;
  desc_line_masks(d, d.variant);
  d.max_levels = d.A + 1;
  return 0;
}

static int build_desc(const char* name, const char* params, Desc* out) {
  static const struct {
    const char* name;
    int (*build)(const char*, const char*, Desc&);
  } games[] = {{"four_to_one", desc_sum},   {"sum_four_to_one", desc_sum},        {"tic_tac_toe_np", desc_ttt},
               {"mttt", desc_ttt},          {"toot_and_otto_bitstring", desc_toot}, {"othello_bit_new", desc_othello},
               {"connect_four", desc_connect}};
  Desc d;
  memset(&d, 0, sizeof d);
  int rc = -1;
  for (const auto& g : games)
    if (!strcmp(name, g.name)) {
      if ((rc = g.build(name, params, d))) return rc;
      break;
    }
  if (rc) return fail(GM_EINVAL, "no device descriptor for game '%s'", name);
  // the checks every game shares
  if (kv(params, "symmetry", 0) && !d.sym)
    return fail(GM_EINVAL, "'%s' defines no symmetry_functions() to reduce by", name);
  if (kv(params, "board_symmetry", 0)) {  // orbit representatives under the board's group (gm_sym.h)
    if (!sym_board_maps(d))
      return fail(GM_EINVAL, "'%s' has no board: board_symmetry=1 covers tic-tac-toe, toot-and-otto, othello and connect four "
                             "(heap permutations are not implemented)", name);
    if (kv(params, "symmetry", 0))
      return fail(GM_EINVAL, "board_symmetry=1 and symmetry=1 do not combine: player_flip swaps the colours "
                             "the board maps keep");
    d.bsym = 1;
    if (d.col0) {  // the gravity boards' mirror: two planes of H rows
      d.nmir = d.L / 2;
      for (int i = 0; i < d.nmir; i++) d.mir[i] = sym_toot_mask(d.L, d.H, i);
    }
    // every map fixes the start position, so the group acts on the reachable
    // set and the root is its own representative
    for (int i = 0; i < sym_board_maps(d); i++)
      if (sym_board_map(d, d.root, i) != d.root)
        return fail(GM_EINVAL, "board map %d of '%s' moves the start position of this board", i, name);
    if (sym_board_canon(d, d.root) != d.root) return fail(GM_EINVAL, "the root of '%s' is not its own representative", name);
  }
  *out = d;
  return 0;
}

static const Desc* get_game(int id) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (id < 0 || id >= (int)g_games.size()) return nullptr;
  return &g_games[id];
}

int gm_game_lookup(const char* name, const char* params, int* game_id) {
  if (!name || !game_id) return fail(GM_EINVAL, "null argument");
  Desc d;
  int rc = build_desc(name, params ? params : "", &d);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  for (size_t i = 0; i < g_games.size(); i++)
    if (!memcmp(&g_games[i], &d, sizeof d)) { *game_id = (int)i; return 0; }
  g_games.push_back(d);
  *game_id = (int)g_games.size() - 1;
  return 0;
}

// Boards whose reachable positions (and, where enumerated, edges) are known:
// SURVEY Appendix B, tests/golden/connect_four/summary.json.  variant -1:
// any; edges 0: not enumerated.  Connect four rows are for connect 4; a
// board with another line length has no row.
struct KnownBoard {
  int kind, L, H, variant;
  u64 positions, edges;
};
static const KnownBoard* known_board(const Desc* d) {
  static const KnownBoard kn[] = {
      {K_TTT, 0, 0, -1, 5478ull, 16167ull},           {K_OTHELLO, 4, 4, -1, 54089ull, 69916ull},
      {K_TOOT, 3, 3, -1, 11097ull, 27774ull},         {K_TOOT, 4, 3, -1, 200127ull, 640648ull},
      {K_TOOT, 3, 4, -1, 126559ull, 0},               {K_TOOT, 4, 4, -1, 3468773ull, 9932808ull},
      {K_TOOT, 5, 4, -1, 70184763ull, 226547754ull},  {K_TOOT, 6, 4, -1, 1187212827ull, 4243234712ull},
      {K_CONNECT, 4, 4, 4, 161029ull, 304574ull},     {K_CONNECT, 5, 4, 4, 3945711ull, 8757625ull}};
  for (const KnownBoard& k : kn)
    if (k.kind == d->kind && k.L == d->L && k.H == d->H && (k.variant < 0 || k.variant == d->variant)) return &k;
  return nullptr;
}

// boards of L columns of 0..H pieces with n pieces in all, times the ways to
// colour them with ceil(n/2) X and floor(n/2) O, summed over n (L*H <= 30:
// every term fits 64 bits)
static uint64_t connect_fillings(int L, int H) {
  const int A = L * H;
  uint64_t ways[31] = {1}, choose[31][31] = {};
  for (int c = 0; c < L; c++) {  // one column more: heights 0..H
    uint64_t next[31] = {};
    for (int n = 0; n <= A; n++)
      for (int h = 0; h <= H && n + h <= A; h++) next[n + h] += ways[n];
    memcpy(ways, next, sizeof ways);
  }
  for (int n = 0; n <= A; n++) {
    choose[n][0] = 1;
    for (int r = 1; r <= n; r++) choose[n][r] = choose[n - 1][r - 1] + (r <= n - 1 ? choose[n - 1][r] : 0);
  }
  uint64_t total = 0;
  for (int n = 0; n <= A; n++) total += ways[n] * choose[n][n / 2];
  return total;
}

// positions bound: the state space of a heap sum; a known board's count;
// for connect four otherwise the gravity fillings with balanced colours, wins
// ignored (a true upper bound); else 0 -- the caller passes an estimate to
// gm_plan
int gm_game_info(int game, uint64_t* positions_bound, uint32_t* max_levels, uint32_t* key_bits) {
  const Desc* d = get_game(game);
  if (!d) return fail(GM_EINVAL, "bad game id %d", game);
  uint64_t bound = 0;
  uint32_t bits = (uint32_t)(2 * d->A + kind_facts(d->kind).key_extra);
  if (d->kind == K_SUM) {
    unsigned __int128 p = 1;
    for (int i = 0; i < d->nheaps; i++) p *= d->base[i];
    bound = (uint64_t)p;
    bits = 64 - __builtin_clzll(bound | 1);
  } else if (const KnownBoard* k = known_board(d)) {
    bound = k->positions;
  } else if (d->kind == K_CONNECT) {
    bound = connect_fillings(d->L, d->H);
  }
  if (positions_bound) *positions_bound = bound;
  if (max_levels) *max_levels = (uint32_t)d->max_levels;
  if (key_bits) *key_bits = bits;
  return 0;
}

int gm_root(int game, uint64_t* key) {
  const Desc* d = get_game(game);
  if (!d || !key) return fail(GM_EINVAL, "bad game id %d", game);
  *key = d->root;
  return 0;
}
