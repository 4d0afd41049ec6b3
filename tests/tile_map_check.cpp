// Stand-alone check of cqa-crct_amd/csrc/tile_map.h (built and run by tests/test_tile_map_cpu.py with the host compiler: no HIP): the
// block -> tile arithmetic of every GEMM launch, walked block by block the way the kernels walk it.
// Prints one "<case> ok" / "<case> FAIL" line per case; the exit status is the number of failures (the first failing input of a case
// goes to stderr).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tile_map.h"

namespace {
using namespace crct;

int failures = 0;
// one case = one property over a whole sweep: fail(...) records the first input that breaks it
struct Case {
  std::string name;
  bool ok = true;
  explicit Case(std::string n) : name(std::move(n)) {}
  template <class... A>
  void fail(const char* fmt, A... a) {
    if (ok) { fprintf(stderr, "%s: ", name.c_str()); fprintf(stderr, fmt, a...); fprintf(stderr, "\n"); }
    ok = false;
  }
  void need(bool cond, const char* what, int a = 0, int b = 0, int c = 0, int d = 0) { if (!cond) fail("%s (%d %d %d %d)", what, a, b, c, d); }
  ~Case() { printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL"); failures += !ok; }
};

struct Shape { int BM, BN; const char* name; };
const Shape kShapes[] = {{128, 128, "128x128"}, {64, 64, "64x64"}, {64, 128, "64x128"}, {128, 64, "128x64"}, {256, 128, "256x128"}};
constexpr int SWEEP = 48;

// an extent of `tiles` tiles of size B: a whole multiple, one element into the last tile, or a ragged last tile -- by turns
int extent(int tiles, int B, int turn) {
  switch (turn % 3) {
    case 0: return tiles * B;
    case 1: return (tiles - 1) * B + 1;
    default: return tiles * B - 7;
  }
}
int ceil_div(int a, int b) { return (a + b - 1) / b; }

uint32_t rng_state = 0x2545F491u;      // fixed seed: the same groups on every run
uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// ------------------------------------------------------------------ single launches
void check_single(const Shape& sh) {
  const std::string p = std::string("single_") + sh.name + "_";
  Case c_grid(p + "grid_is_8_rectangles"), c_count(p + "true_count_is_tile_count"), c_once(p + "every_tile_exactly_once"),
      c_rest(p + "every_other_block_false");
  std::vector<uint8_t> seen;
  for (int tm_n = 1; tm_n <= SWEEP; ++tm_n)
    for (int tn_n = 1; tn_n <= SWEEP; ++tn_n)
      for (int turn = 0; turn < 3; ++turn) {
        const int M = extent(tm_n, sh.BM, turn), N = extent(tn_n, sh.BN, turn + tm_n);
        int grid = -1;
        const TileMap t = make_tile_map(M, N, sh.BM, sh.BN, &grid);
        c_grid.need(t.tiles_m == tm_n && t.tiles_n == tn_n, "tile counts", M, N, t.tiles_m, t.tiles_n);
        const bool gn_ok = t.gn == 1 || t.gn == 2 || t.gn == 4 || t.gn == 8;
        c_grid.need(gn_ok, "gn divides 8", M, N, t.gn);
        if (!gn_ok) continue;
        const int gm = 8 / t.gn;
        c_grid.need(gm * t.gn == 8 && t.rm == ceil_div(tm_n, gm) && t.rn == ceil_div(tn_n, t.gn) && grid == 8 * t.rm * t.rn, "gm * gn == 8, grid == 8 * rm * rn",
                    M, N, grid, t.gn);
        seen.assign((size_t)tm_n * tn_n, 0);
        int trues = 0;
        for (int bid = 0; bid < grid; ++bid) {
          int tm = -1, tn = -1;
          if (!map_tile(t, bid, tm, tn)) continue;
          ++trues;
          if (tm < 0 || tm >= tm_n || tn < 0 || tn >= tn_n) { c_once.fail("tile out of range: M %d N %d bid %d -> (%d, %d)", M, N, bid, tm, tn); continue; }
          if (seen[(size_t)tm * tn_n + tn]++) c_once.fail("tile twice: M %d N %d bid %d -> (%d, %d)", M, N, bid, tm, tn);
        }
        for (size_t i = 0; i < seen.size(); ++i)
          if (!seen[i]) c_once.fail("tile skipped: M %d N %d tile %d", M, N, (int)i);
        c_count.need(trues == tm_n * tn_n, "true blocks", M, N, trues, grid);
        // what is not a tile of the map is no tile at all: the padding blocks inside the grid (counted above) and everything behind it
        for (int bid = grid; bid < grid + 64; ++bid) {
          int tm, tn;
          c_rest.need(!map_tile(t, bid, tm, tn), "block behind the grid maps to a tile", M, N, bid, grid);
        }
        c_rest.need(grid - trues == grid - tm_n * tn_n && grid >= tm_n * tn_n, "padding blocks", M, N, trues, grid);
      }
}

// ------------------------------------------------------------------ K-partitioned launches
void check_splitk(const Shape& sh) {
  const std::string p = std::string("splitk_") + sh.name + "_";
  Case c_once(p + "every_tile_slice_exactly_once"), c_xcd(p + "slices_of_a_tile_share_an_xcd"), c_ticket(p + "ticket_inside_ticket_array"),
      c_slab(p + "slabs_inside_workspace");
  std::vector<uint8_t> seen;
  std::vector<int> xcd;
  for (int tm_n = 1; tm_n <= SWEEP; ++tm_n)
    for (int tn_n = 1; tn_n <= SWEEP; ++tn_n)
      for (int S = 2; S <= 8; ++S) {
        const int M = extent(tm_n, sh.BM, tm_n + S), N = extent(tn_n, sh.BN, tn_n + tm_n);
        int grid = -1;
        const TileMap t = make_tile_map(M, N, sh.BM, sh.BN, &grid);
        const int tiles = tm_n * tn_n, tickets = splitk_tickets(M, N);
        const int64_t ws = splitk_ws_elems(M, N, S);
        seen.assign((size_t)tiles * S, 0);
        xcd.assign(tiles, -1);
        for (unsigned bid = 0; bid < (unsigned)grid * S; ++bid) {
          int tm = -1, tn = -1, slice = -1, lin = -1;
          if (!map_splitk(t, bid, S, tm, tn, slice, lin)) continue;
          if (tm < 0 || tm >= tm_n || tn < 0 || tn >= tn_n || slice < 0 || slice >= S || lin != tm * tn_n + tn) {
            c_once.fail("out of range: M %d N %d S %d bid %u -> (%d, %d) slice %d lin %d", M, N, S, bid, tm, tn, slice, lin);
            continue;
          }
          if (seen[(size_t)lin * S + slice]++) c_once.fail("twice: M %d N %d S %d bid %u -> tile %d slice %d", M, N, S, bid, lin, slice);
          if (xcd[lin] < 0) xcd[lin] = bid & 7;
          c_xcd.need(xcd[lin] == (int)(bid & 7), "slices on two XCDs", M, N, S, lin);
          c_ticket.need(lin >= 0 && lin < tickets, "tile_lin >= tickets", M, N, lin, tickets);
          if ((int64_t)(lin + 1) * S * sh.BM * sh.BN > ws) c_slab.fail("M %d N %d S %d: slabs of tile %d end at %lld of %lld elements", M, N, S, lin,
                                                                        (long long)((int64_t)(lin + 1) * S * sh.BM * sh.BN), (long long)ws);
        }
        for (size_t i = 0; i < seen.size(); ++i)
          if (!seen[i]) c_once.fail("skipped: M %d N %d S %d tile %d slice %d", M, N, S, (int)(i / S), (int)(i % S));
      }
  Case c_zero(p + "no_workspace_unsplit");
  c_zero.need(splitk_ws_elems(1000, 1000, 1) == 0 && splitk_ws_elems(1000, 1000, 0) == 0, "split_k <= 1 needs no slabs");
}

// ------------------------------------------------------------------ grouped launches
struct Problem { int M, N; };
using Group = std::vector<Problem>;

// position of (tm, tn) in the concatenated tile list, from its definition: problem after problem, inside a problem along its shorter
// grid dimension first
int list_index(const GroupPlace& ga, int pi, int tm, int tn) {
  int before = 0;
  for (int i = 0; i < pi; ++i) before += ga.map[i].tiles_m * ga.map[i].tiles_n;
  const int nm = ga.map[pi].tiles_m, nn = ga.map[pi].tiles_n;
  return before + (nn <= nm ? tm * nn + tn : tn * nm + tm);
}

struct GroupCases {
  Case begin8, once, c_total, c_once, c_run, c_pad;
  explicit GroupCases(const std::string& p)
      : begin8(p + "problems_begin_on_xcd_0"), once(p + "default_every_tile_exactly_once"), c_total(p + "concat_total_is_8_per_xcd"),
        c_once(p + "concat_every_tile_exactly_once"), c_run(p + "concat_xcd_owns_one_run_of_the_list"), c_pad(p + "concat_padding_blocks_false") {}
};

// walks [0, total) in both modes; returns the default-mode total
int check_group(const Group& g, const Shape& sh, GroupCases& c, std::vector<int>* totals) {
  const int n = (int)g.size();
  GroupPlace ga = {};
  ga.n = n;
  int total = 0, tiles = 0;
  std::vector<int> first(n + 1, 0);      // first tile of every problem in one flat "seen" array
  for (int i = 0; i < n; ++i) {
    group_add(ga, i, g[i].M, g[i].N, sh.BM, sh.BN, &total);
    first[i] = tiles;
    tiles += ga.map[i].tiles_m * ga.map[i].tiles_n;
  }
  first[n] = tiles;
  for (int i = 0; i <= n; ++i) c.begin8.need(ga.tile_begin[i] % 8 == 0, "tile_begin % 8", n, i, ga.tile_begin[i]);
  c.begin8.need(ga.tile_begin[n] == total && group_total(ga) == total, "tile_begin[n] is the total", n, total, ga.tile_begin[n]);
  auto slot = [&](int pi, int tm, int tn) -> int {
    if (pi < 0 || pi >= n || tm < 0 || tm >= ga.map[pi].tiles_m || tn < 0 || tn >= ga.map[pi].tiles_n) return -1;
    return first[pi] + tm * ga.map[pi].tiles_n + tn;
  };
  std::vector<uint8_t> seen(tiles, 0);
  for (int bid = 0; bid < total; ++bid) {
    int pi = -1, tm = -1, tn = -1;
    if (!group_pick(ga, bid, pi, tm, tn)) continue;
    const int s = slot(pi, tm, tn);
    if (s < 0) c.once.fail("n %d bid %d -> problem %d tile (%d, %d) out of range", n, bid, pi, tm, tn);
    else if (seen[s]++) c.once.fail("n %d bid %d -> problem %d tile (%d, %d) twice", n, bid, pi, tm, tn);
  }
  for (int s = 0; s < tiles; ++s)
    if (!seen[s]) c.once.fail("n %d: tile %d of the group skipped (first problem %d x %d)", n, s, g[0].M, g[0].N);
  if (totals) totals->push_back(total);

  // concat mode on the same group
  int ctotal = total;
  group_concat(ga, &ctotal);
  c.c_total.need(ctotal == 8 * ga.per_xcd && group_total(ga) == ctotal && ctotal >= tiles && ctotal < tiles + 8 && ga.tile_prefix[n] == tiles,
                 "total == 8 * per_xcd == tiles rounded up to 8", n, ctotal, ga.per_xcd, tiles);
  if (totals) totals->push_back(ctotal);
  seen.assign(tiles, 0);
  int falses = 0;
  for (int x = 0; x < 8; ++x) {
    int run_first = -1, run_len = 0;
    bool ended = false;
    for (int j = 0; 8 * j + x < ctotal; ++j) {
      const int bid = 8 * j + x;
      int pi = -1, tm = -1, tn = -1;
      if (!group_pick(ga, bid, pi, tm, tn)) { ++falses; ended = true; continue; }
      const int s = slot(pi, tm, tn);
      if (s < 0) { c.c_once.fail("n %d bid %d -> problem %d tile (%d, %d) out of range", n, bid, pi, tm, tn); continue; }
      if (seen[s]++) c.c_once.fail("n %d bid %d -> problem %d tile (%d, %d) twice", n, bid, pi, tm, tn);
      const int li = list_index(ga, pi, tm, tn);
      if (run_first < 0) run_first = li;
      c.c_run.need(!ended && li == run_first + run_len, "the blocks of an XCD are not one run of consecutive list entries", n, x, j, li);
      ++run_len;
    }
    c.c_run.need(run_len <= ga.per_xcd, "run longer than per_xcd", n, x, run_len, ga.per_xcd);
  }
  for (int s = 0; s < tiles; ++s)
    if (!seen[s]) c.c_once.fail("n %d: tile %d of the group skipped in concat mode", n, s);
  c.c_pad.need(falses == ctotal - tiles, "padding blocks", n, falses, ctotal, tiles);
  for (int bid = ctotal; bid < ctotal + 64; ++bid) {      // a persistent walk never goes there; no tile may be behind the grid all the same
    int pi, tm, tn;
    c.c_pad.need(!group_pick(ga, bid, pi, tm, tn), "block behind the grid maps to a tile", n, bid, ctotal);
  }
  return total;
}

void check_groups(std::vector<int>* totals) {
  for (const Shape& sh : {kShapes[0], kShapes[3]}) {      // 128x128: every grouped configuration that is built; 128x64: a non-square tile
    GroupCases c(std::string("group_") + sh.name + "_");
    Case special(std::string("group_") + sh.name + "_edge_groups_present");
    bool had_1x1 = false, had_small = false, had_ragged = false;
    for (int n = 1; n <= GROUP_MAX; ++n) {
      // every problem one tile (fewer than 8 tiles in all, and for n < 8 a total that is no multiple of 8)
      Group ones;
      for (int i = 0; i < n; ++i) ones.push_back({1 + (int)(rng() % sh.BM), 1 + (int)(rng() % sh.BN)});
      check_group(ones, sh, c, totals);
      had_1x1 = true;
      // fewer than 8 tiles in total although a problem has several
      if (n <= 6) {
        Group few = ones;
        few[0] = {sh.BM * (8 - n) - 3, sh.BN};      // (8 - n) x 1 tiles beside n - 1 single ones: 7 in all
        check_group(few, sh, c, totals);
        had_small = true;
      }
      for (int rep = 0; rep < 150; ++rep) {
        Group g;
        int tiles = 0;
        for (int i = 0; i < n; ++i) {
          // small problems mostly (the weight gradients of a layer are 6 x 6 .. 24 x 6 tiles), now and then up to 48 tiles a side
          const int lim_m = (rng() % 4 == 0) ? SWEEP : 9, lim_n = (rng() % 4 == 0) ? SWEEP : 9;
          const int tm = 1 + (int)(rng() % lim_m), tn = 1 + (int)(rng() % lim_n);
          g.push_back({extent(tm, sh.BM, (int)(rng() % 3)), extent(tn, sh.BN, (int)(rng() % 3))});
          tiles += tm * tn;
        }
        had_ragged = had_ragged || tiles % 8 != 0;
        check_group(g, sh, c, totals);
      }
    }
    special.need(had_1x1 && had_small && had_ragged, "all 1x1 / fewer than 8 tiles / a total that is no multiple of 8");
  }
}

// ------------------------------------------------------------------ the grid of a grouped launch
void check_group_grid(const std::vector<int>& group_totals) {
  Case c_range("group_grid_between_1_and_total"), c_8("group_grid_multiple_of_8_or_total"), c_rounds("group_grid_target_keeps_the_rounds"),
      c_xcd("group_grid_walk_stays_on_one_xcd"), c_cap("group_grid_cap_overrides_target"), c_other("group_grid_other_kinds_ignore_target_obey_cap");
  std::vector<int> totals = group_totals;
  for (int k = 1; k <= 320; ++k) totals.push_back(8 * k);
  std::sort(totals.begin(), totals.end());
  totals.erase(std::unique(totals.begin(), totals.end()), totals.end());
  for (int total : totals) {
    const int knobs[] = {0, 1, 7, 8, 9, 95, 96, 97, total - 1, total, total + 1};
    for (int target : knobs)
      for (int cap_in : knobs) {
        const int cap = group_cap(cap_in);
        for (int wgrad = 0; wgrad < 2; ++wgrad) {
          const int grid = group_grid(total, target, wgrad != 0, cap);
          c_range.need(grid > 0 && grid <= total, "0 < grid <= total", total, target, cap_in, grid);
          c_8.need(grid % 8 == 0 || grid == total, "grid % 8", total, target, cap_in, grid);
          if (grid <= 0) continue;
          if (wgrad && target > 0 && cap == 0)
            c_rounds.need(ceil_div(total, grid) <= ceil_div(total, target), "more rounds than the target asks for", total, target, grid);
          if (grid % 8 == 0 && (target == knobs[0] || target == 96))      // the walk b, b + grid, ... of every workgroup (two targets: the walk depends on grid alone)
            for (int b = 0; b < grid; ++b)
              for (int bid = b; bid < total; bid += grid) c_xcd.need((bid & 7) == (b & 7), "walk changes XCD", total, grid, b, bid);
          if (cap > 0) {
            c_cap.need(grid == (cap < total ? cap : total), "cap", total, target, cap, grid);
            c_cap.need(cap % 8 == 0 && cap >= cap_in && cap < cap_in + 8, "cap rounded up to 8", cap_in, cap);
          } else {
            c_cap.need(cap_in <= 0, "a positive cap was dropped", cap_in, cap);
          }
          if (!wgrad) c_other.need(grid == (cap > 0 && cap < total ? cap : total), "forward / data gradient / fp8", total, target, cap, grid);
        }
      }
  }
}
}  // namespace

int main() {
  for (const Shape& sh : kShapes) check_single(sh);
  check_splitk(kShapes[0]);      // the tiles of the K-partitioned configurations: 128x128 (4, 9) and 128x64 (12, 15)
  check_splitk(kShapes[3]);
  std::vector<int> totals;
  check_groups(&totals);
  check_group_grid(totals);
  return failures > 255 ? 255 : failures;
}
