// Where every GEMM workgroup goes: the integer arithmetic that takes a block index to its output tile -- single launches (make_tile_map /
// map_tile), K-partitioned launches (map_splitk, with the sizes of their slab space and ticket array), grouped launches (GroupPlace,
// group_add / group_pick / group_concat) and the size of a grouped launch's grid (group_grid).  Nothing from HIP in here: gemm.hip
// includes this header and its kernels and launchers call these functions; tests/tile_map_check.cpp compiles the same definitions with
// the host compiler and checks them block by block (tests/test_tile_map_cpu.py).  A tile skipped or visited twice is a wrong result;
// a ticket or slab index past its buffer corrupts a neighbouring one.
#pragma once
#include <stdint.h>

#include "crct_hip.h"      // CrctGemmLnAddend (plain C)

#if defined(__HIPCC__)
#define CRCT_TILE_FN __host__ __device__ __forceinline__
#define CRCT_TILE_UNROLL _Pragma("unroll")
#else
#define CRCT_TILE_FN inline
#define CRCT_TILE_UNROLL
#endif

namespace crct {

// ------------------------------------------------------------------ XCD-aware tile placement
// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD group, each with a
// private 4 MiB L2).  The tile grid is cut into gm x gn = 8 rectangles, one per XCD, chosen so that
// the A' and B' panels one XCD touches (rm*BM + rn*BN rows of K) are as few as possible and stay
// L2-resident; block j of XCD x takes the j-th tile of rectangle x.  Placement only affects speed.
struct TileMap { int tiles_m, tiles_n, gn, rm, rn, dbg; CrctGemmLnAddend lna; };   // dbg: ablation bits of the -DCRCT_GEMM_LAB build (tools/gemm_lab); the shipped library ignores them

CRCT_TILE_FN int tile_min(int a, int b) { return a < b ? a : b; }

CRCT_TILE_FN bool map_tile(const TileMap& t, int bid, int& tm, int& tn) {
  const int x = bid & 7, j = bid >> 3;
  const int m_lo = (x / t.gn) * t.rm, n_lo = (x % t.gn) * t.rn;
  const int hm = tile_min(t.rm, t.tiles_m - m_lo), hn = tile_min(t.rn, t.tiles_n - n_lo);
  if (hm <= 0 || hn <= 0 || j >= hm * hn) return false;
  tm = m_lo + j / hn;
  tn = n_lo + j % hn;
  return true;
}

// the map of an M x N output in BM x BN tiles and its grid (8 * rm * rn blocks); dbg = 0, no LayerNorm addend
CRCT_TILE_FN TileMap make_tile_map(int M, int N, int BM, int BN, int* grid) {
  TileMap t;
  t.tiles_m = (M + BM - 1) / BM; t.tiles_n = (N + BN - 1) / BN;
  long best = -1;
  int bgm = 1;
  for (int gm = 1; gm <= 8; gm *= 2) {
    const int gn = 8 / gm;
    const int rm = (t.tiles_m + gm - 1) / gm, rn = (t.tiles_n + gn - 1) / gn;
    // panel rows held per XCD, plus a penalty for padded (idle) blocks
    const long cost = (long)rm * BM + (long)rn * BN + 4L * ((long)rm * rn * 8 - (long)t.tiles_m * t.tiles_n) * 16;
    if (best < 0 || cost < best) { best = cost; bgm = gm; }
  }
  t.gn = 8 / bgm;
  t.rm = (t.tiles_m + bgm - 1) / bgm; t.rn = (t.tiles_n + t.gn - 1) / t.gn;
  *grid = 8 * t.rm * t.rn;
  t.dbg = 0;
  t.lna = CrctGemmLnAddend{nullptr, nullptr, nullptr, nullptr};
  return t;
}

// K-partitioned launch: block j of XCD x is slice j % S of the (j / S)-th tile of that XCD's rectangle -- a tile's slices share
// an L2 (speed only).  Grid = 8 * rm * rn * S.  tile_lin: the tile's ticket and the first of its S slabs.
CRCT_TILE_FN int splitk_block(unsigned bid, int S) {      // the block of the unsplit map whose tile `bid` works on
  const int x = bid & 7, j = bid >> 3;
  return ((j / S) << 3) | x;
}
CRCT_TILE_FN int splitk_slice(unsigned bid, int S) { const int j = bid >> 3; return j % S; }
CRCT_TILE_FN int splitk_tile_lin(const TileMap& t, int tm, int tn) { return tm * t.tiles_n + tn; }
// ... together (gemm_splitk_kernel takes the same three steps)
CRCT_TILE_FN bool map_splitk(const TileMap& t, unsigned bid, int S, int& tm, int& tn, int& slice, int& tile_lin) {
  if (!map_tile(t, splitk_block(bid, S), tm, tn)) return false;
  slice = splitk_slice(bid, S);
  tile_lin = splitk_tile_lin(t, tm, tn);
  return true;
}
// split-K needs the LDS-DMA kernel; the slab space (fp32 elements) is sized for the larger of the tiles it is built with (128 x 128)
CRCT_TILE_FN int64_t splitk_ws_elems(int M, int N, int split_k) {
  if (split_k <= 1) return 0;
  const int64_t tm = (M + 127) / 128, tn = (N + 127) / 128;
  return tm * tn * 128 * 128 * (int64_t)split_k;
}
// ... and one ticket per tile of the smaller one (128 x 64)
CRCT_TILE_FN int splitk_tickets(int M, int N) { return ((M + 127) / 128) * ((N + 63) / 64); }

// ---- grouped launch: up to 8 independent GEMMs of the same mode in ONE grid (the weight gradients of one
// layer: 4-6 small problems that individually leave most CUs idle).  Block -> (problem, tile) by prefix table.
constexpr int GROUP_MAX = 8;
struct GroupPlace {
  int n;
  int tile_begin[GROUP_MAX + 1];       // first block of every problem (multiples of 8: a problem starts on XCD 0)
  TileMap map[GROUP_MAX];              // per-problem XCD-aware block -> tile map, as for single launches
  // concat != 0 (the weight gradients of a layer): the tiles of ALL problems form one list -- problem after problem, inside a
  // problem along its shorter grid dimension first -- and XCD x (= block % 8) takes the x-th run of per_xcd consecutive tiles.  A
  // run then lies inside one or two problems and covers a compact rectangle of each: an XCD's private L2 fetches the operand
  // panels of ~1/8 of the group instead of 1/8 of EVERY problem (fabric reads of a text layer's group 143 -> ~50 MB).
  int concat, per_xcd;
  int tile_prefix[GROUP_MAX + 1];      // tiles before every problem (concat mode)
};
// block -> (problem, tile) of a grouped launch; false: a padding block
CRCT_TILE_FN bool group_pick(const GroupPlace& ga, int bid, int& pi, int& tm, int& tn) {
  pi = 0;
  if (ga.concat) {
    const int j = bid >> 3, t = (bid & 7) * ga.per_xcd + j;
    if (j >= ga.per_xcd || t >= ga.tile_prefix[ga.n]) return false;
    CRCT_TILE_UNROLL
    for (int i = 1; i < GROUP_MAX; ++i)
      if (i < ga.n && t >= ga.tile_prefix[i]) pi = i;
    const int local = t - ga.tile_prefix[pi], nm = ga.map[pi].tiles_m, nn = ga.map[pi].tiles_n;
    if (nn <= nm) { tm = local / nn; tn = local - tm * nn; }
    else { tn = local / nm; tm = local - tn * nm; }
    return true;
  }
  CRCT_TILE_UNROLL
  for (int i = 1; i < GROUP_MAX; ++i)
    if (i < ga.n && bid >= ga.tile_begin[i]) pi = i;
  return map_tile(ga.map[pi], bid - ga.tile_begin[pi], tm, tn);
}
// problem i of a group under construction: its map behind the blocks of the problems before it; *total: the blocks so far
CRCT_TILE_FN void group_add(GroupPlace& ga, int i, int M, int N, int BM, int BN, int* total) {
  ga.tile_begin[i] = *total;
  int blocks = 0;
  ga.map[i] = make_tile_map(M, N, BM, BN, &blocks);
  *total += blocks;
  ga.tile_begin[i + 1] = *total;
}
CRCT_TILE_FN void group_concat(GroupPlace& ga, int* grid) {      // host side of concat mode
  int tiles = 0;
  for (int i = 0; i < ga.n; ++i) { ga.tile_prefix[i] = tiles; tiles += ga.map[i].tiles_m * ga.map[i].tiles_n; }
  ga.tile_prefix[ga.n] = tiles;
  ga.concat = 1;
  ga.per_xcd = (tiles + 7) / 8;
  *grid = 8 * ga.per_xcd;
}
// the blocks a grouped kernel walks: workgroup b takes blocks b, b + gridDim, ... below this
CRCT_TILE_FN int group_total(const GroupPlace& ga) { return ga.concat ? 8 * ga.per_xcd : ga.tile_begin[ga.n]; }

// Workgroups of a grouped launch over `total` blocks.  max_wgs > 0 (crct_gemm_group_max_workgroups, a multiple of 8) caps every grouped
// launch and overrides the target.  Otherwise a bf16 weight-gradient group with a target walks the block list in whole rounds --
// rounds = ceil(total / target), grid = ceil(total / rounds) rounded up to the 8 XCDs; everything else runs one workgroup per block.
// A grid smaller than `total` makes the workgroups persistent; a grid that is a multiple of 8 keeps a workgroup's blocks on one XCD.
CRCT_TILE_FN int group_cap(int n) { return n > 0 ? (n + 7) / 8 * 8 : 0; }      // what crct_gemm_group_max_workgroups(n) keeps as max_wgs
CRCT_TILE_FN int group_grid(int total, int target, bool wgrad_bf16, int max_wgs) {
  if (max_wgs > 0) return max_wgs < total ? max_wgs : total;
  if (!wgrad_bf16 || target <= 0 || total <= target) return total;
  const int rounds = (total + target - 1) / target;
  const int grid = ((total + rounds - 1) / rounds + 7) / 8 * 8;
  return grid < total ? grid : total;
}

}  // namespace crct
