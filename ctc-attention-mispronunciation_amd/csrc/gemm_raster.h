// The order in which the persistent workgroups of gemm_f32x6_kernel (gemm_bf16x6.hip) take the tiles of C -- 256 x 128 (four 16-row MFMA
// tiles per wave, RT = 4) or 192 x 128 (RT = 3) -- : one function from (workgroup, round) to a tile, and the host-side rules that choose
// between the two walks and between the two tiles.  Host only, like plan.h: no HIP type, no device
// code of its own (tests/test_gemm_raster_host.py builds it with the host compiler and walks every shape); the kernel calls x6_tile_of
// once per tile, in scalar code.
//
// Workgroup wg runs on XCD wg % 8 (workgroups are dealt to the eight XCDs in turn), and an XCD's workgroups move through K in step, so
// what one XCD's workgroups work on in a round is what its 4 MiB L2 has to hold a K-tile of at a time.
//   row walk    each XCD takes a contiguous run of row-major tiles, its workgroup j of round r the run's tile r * (grid / 8) + j.  At
//               24 column tiles a round of 32 workgroups spans every column tile and two or three row panels: per round the XCD
//               pulls the whole of W and two or three A panels through its L2.
//   block walk  tiles in blocks of rb row panels x cb column tiles (smaller at the right and bottom edge), the blocks row-major and
//               dealt to the XCDs in turn: block r * 8 + xcd is the XCD's round r, its workgroup j takes the block's tile j (row-major
//               in the block), and a workgroup whose j is past a short block's size sits that round out.  Per round the XCD pulls
//               cb column tiles of W and rb A panels: rb * cb = 32 minimises 256 rb + 128 cb (RT = 3: 192 rb + 128 cb) near 4 x 8.  Needs a
//               grid of 8 x 32.
// Either walk gives a tile to exactly one (workgroup, round), and a C element's own K order does not depend on the walk: the outputs
// are the same bits.  Nor does it depend on the tile: RT = 4 performs RT = 3's arithmetic on every element.
#pragma once
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#define MDD_RASTER_HD __host__ __device__
#else
#define MDD_RASTER_HD
#endif

namespace mdd {

constexpr int kX6Xcds = 8, kX6WgPerXcd = 32, kX6Grid = kX6Xcds * kX6WgPerXcd;   // one persistent workgroup per CU of the device

// rb == 0: the row walk.  Otherwise rb x cb blocks, rb * cb <= 32.
struct X6Raster { int rb, cb; };
constexpr X6Raster kX6Rows = {0, 0};
constexpr X6Raster kX6DefaultRaster = {4, 8};   // profiles/gemm_raster_notes.txt, profiles/gemm_rt4_notes.txt

// Rows of C per workgroup tile: four waves of RT 16-row MFMA tiles each.
constexpr int x6_bm(int rt) { return 4 * 16 * rt; }
// MDD_GEMM_X6_RT: "3" or "4" is that tile in every launch that takes the switch; unset, x6_choose_tile's rule decides per launch (kX6RtRule).
// x6_rt_parse: false for any other value (the mdd_diag_gemm* entries refuse it, as they refuse a mistyped walk); x6_rt_from_env: a handle's
// reading at create, where any other value is the default.
constexpr int kX6RtRule = 0;
inline bool x6_rt_parse(const char *e, int *out) {
    if (!e || (strcmp(e, "3") && strcmp(e, "4"))) return false;
    *out = e[0] - '0';
    return true;
}
inline int x6_rt_from_env(const char *e) {
    int rt = kX6RtRule;
    if (e) x6_rt_parse(e, &rt);
    return rt;
}

// MDD_GEMM_X6_RASTER: "rows" is the row walk everywhere; "<rb>x<cb>" (2x16, 4x8, 8x4: the timing aid's arms) those blocks, rb * cb <= 32.
// x6_raster_parse: false for any other value (the mdd_diag_gemm* entries refuse it: a mistyped arm of an A/B must not run as the default
// under another name).  x6_raster_from_env: what a handle reads at create, where any other value of a switch, or none, is its default (plan.h).
inline bool x6_raster_parse(const char *e, X6Raster *out) {
    if (!e) return false;
    if (!strcmp(e, "rows")) { *out = kX6Rows; return true; }
    char *end = nullptr;
    const long rb = strtol(e, &end, 10);
    if (end == e || *end != 'x') return false;
    const char *c = end + 1;
    const long cb = strtol(c, &end, 10);
    if (end == c || *end || rb < 1 || cb < 1 || rb * cb > kX6WgPerXcd) return false;
    *out = {(int)rb, (int)cb};
    return true;
}
inline X6Raster x6_raster_from_env(const char *e) {
    X6Raster r = kX6DefaultRaster;
    if (e) x6_raster_parse(e, &r);
    return r;
}

// One launch's walk: what the kernel needs to find its tiles.  ntiles == tiles_m * tiles_n.
struct X6Walk {
    int ntiles, tiles_n;
    int rb, cb;     // rb == 0: the row walk
    int grid;       // workgroups launched: min(ntiles, 256) in the row walk, 256 in the block walk
    int rounds;     // rounds r = 0 .. rounds - 1 hold every tile
};

MDD_RASTER_HD inline int x6_ceil_div(int a, int b) { return (a + b - 1) / b; }

// The walk of a tiles_m x tiles_n launch under `want`.  The row walk where the block walk would be the longer one in rounds (9 panels x 24
// column tiles: one round in rows, two in 4 x 8 blocks), where the launch is narrower than a block or smaller than one XCD's round, and
// where `want` says so.
inline X6Walk x6_choose_walk(int tiles_m, int tiles_n, X6Raster want) {
    const int ntiles = tiles_m * tiles_n, row_grid = ntiles < kX6Grid ? ntiles : kX6Grid, row_rounds = x6_ceil_div(ntiles, row_grid);
    const X6Walk rows = {ntiles, tiles_n, 0, 0, row_grid, row_rounds};
    if (want.rb < 1 || want.cb < 1 || want.rb * want.cb > kX6WgPerXcd) return rows;
    if (tiles_n < want.cb || ntiles < kX6WgPerXcd) return rows;
    const int rounds = x6_ceil_div(x6_ceil_div(tiles_m, want.rb) * x6_ceil_div(tiles_n, want.cb), kX6Xcds);
    if (rounds > row_rounds) return rows;
    return {ntiles, tiles_n, want.rb, want.cb, kX6Grid, rounds};
}

// Which tile a launch of M rows x tiles_n column tiles takes, and its walk.  A round costs MFMA time in proportion to RT (every workgroup
// of it multiplies RT x 8 MFMA tiles per K-tile), so RT = 4 is taken where its rounds are no more MFMA time than RT = 3's:
// 4 x rounds(RT = 4) <= 3 x rounds(RT = 3), each counted in the walk that tile would get.  There the larger tile only saves: a quarter of
// the W fragment reads, LDS-DMA bytes and W bytes from beyond L2 per MFMA, and the per-K-tile fixed cost spread over a third more MFMAs
// (profiles/gemm_rt4_notes.txt).  A launch that RT = 3 finishes in one round (the text table's 44 rows, a short utterance's projections)
// therefore stays on RT = 3, where more workgroups share its rows.  rt == 3 or 4 (MDD_GEMM_X6_RT): that tile whatever the counts.
struct X6Tile { int rt; X6Walk walk; };
inline X6Tile x6_choose_tile(int M, int tiles_n, X6Raster want, int rt = kX6RtRule) {
    const X6Walk w3 = x6_choose_walk(x6_ceil_div(M, x6_bm(3)), tiles_n, want), w4 = x6_choose_walk(x6_ceil_div(M, x6_bm(4)), tiles_n, want);
    if (rt == kX6RtRule) rt = 4 * w4.rounds <= 3 * w3.rounds ? 4 : 3;
    return rt == 4 ? X6Tile{4, w4} : X6Tile{3, w3};
}

// Tile (tm, tn) of workgroup wg in round r; false: the workgroup has no tile in that round.  (In the row walk a workgroup's tiles
// end at the first such round; in the block walk it may only be sitting out a short block.)
MDD_RASTER_HD inline bool x6_tile_of(const X6Walk &w, int wg, int r, int &tm, int &tn) {
    const int xcd = wg & (kX6Xcds - 1), j = wg >> 3;
    if (w.rb == 0) {
        const int vb = wg + r * w.grid;
        if (vb >= w.ntiles) return false;
        const int tq = w.ntiles >> 3, trem = w.ntiles & 7;   // an XCD's run: tq tiles, one more on the first trem
        const int vt = (xcd < trem ? xcd * (tq + 1) : trem * (tq + 1) + (xcd - trem) * tq) + (vb >> 3);
        tm = vt / w.tiles_n; tn = vt % w.tiles_n;
        return true;
    }
    const int tiles_m = w.ntiles / w.tiles_n, nbc = x6_ceil_div(w.tiles_n, w.cb), nbr = x6_ceil_div(tiles_m, w.rb);
    const int b = r * kX6Xcds + xcd;
    if (b >= nbr * nbc) return false;
    const int br = b / nbc, bc = b % nbc;
    const int h = tiles_m - br * w.rb < w.rb ? tiles_m - br * w.rb : w.rb, wd = w.tiles_n - bc * w.cb < w.cb ? w.tiles_n - bc * w.cb : w.cb;
    if (j >= h * wd) return false;
    tm = br * w.rb + j / wd; tn = bc * w.cb + j % wd;
    return true;
}

}  // namespace mdd
