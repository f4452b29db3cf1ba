"""csrc/gemm_raster.h with the host compiler: the tile walk of gemm_f32x6_kernel, every shape the projection GEMM can be launched at.

The walk only decides which workgroup computes which 192 x 128 tile of C and when; a slip in it is a tile computed twice, never, or
outside the matrix.  The driver walks every (row panels 1..700) x (column tiles 1..24) at the launch grid of 256 -- the forward's own
667 x 24 and 107 x 24 and the text table's 1 x 24 among them -- under the default walk, the row walk the switch restores, and the two
neighbouring block shapes the timing aid compares."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")

_DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "plan.h"
using namespace mdd;

// The row walk as gemm_f32x6_kernel had it before the walk moved to gemm_raster.h, written out: virtual block vb = blockIdx.x + k * gridDim.x
// of a grid of min(ntiles, 256), XCD vb % 8 walking a contiguous run of row-major tiles.
static void old_tile_of(int ntiles, int tiles_n, int vb, int &tm, int &tn) {
    const int tq = ntiles >> 3, trem = ntiles & 7;
    const int xcd = vb & 7;
    const int vt = (xcd < trem ? xcd * (tq + 1) : trem * (tq + 1) + (xcd - trem) * tq) + (vb >> 3);
    tm = vt / tiles_n; tn = vt % tiles_n;
}

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static void walk_shape(int tiles_m, int tiles_n, X6Raster want, const char *name) {
    const int ntiles = tiles_m * tiles_n;
    const X6Walk w = x6_choose_walk(tiles_m, tiles_n, want);
    const int row_grid = ntiles < 256 ? ntiles : 256, row_rounds = (ntiles + row_grid - 1) / row_grid;
    // the fallback rule, from the shape alone
    bool rows = want.rb == 0;
    if (!rows) {
        const int blocks = ((tiles_m + want.rb - 1) / want.rb) * ((tiles_n + want.cb - 1) / want.cb);
        rows = tiles_n < want.cb || ntiles < 32 || (blocks + 7) / 8 > row_rounds;
    }
    CHECK((w.rb == 0) == rows, "%s %d x %d: walk rb %d, the rule says %s", name, tiles_m, tiles_n, w.rb, rows ? "rows" : "blocks");
    CHECK(w.ntiles == ntiles && w.tiles_n == tiles_n, "%s %d x %d: ntiles %d tiles_n %d", name, tiles_m, tiles_n, w.ntiles, w.tiles_n);
    CHECK(w.grid == (w.rb ? 256 : row_grid), "%s %d x %d: grid %d", name, tiles_m, tiles_n, w.grid);
    CHECK(w.rb == 0 || (w.rb == want.rb && w.cb == want.cb), "%s %d x %d: blocks %d x %d", name, tiles_m, tiles_n, w.rb, w.cb);
    CHECK(w.rounds >= 1 && w.rounds <= row_rounds, "%s %d x %d: %d rounds, the row walk takes %d", name, tiles_m, tiles_n, w.rounds, row_rounds);
    std::vector<int> seen(ntiles, 0);
    for (int r = 0; r <= w.rounds; r++) {
        int lo_m[8], hi_m[8], lo_n[8], hi_n[8];
        for (int x = 0; x < 8; x++) { lo_m[x] = lo_n[x] = 1 << 30; hi_m[x] = hi_n[x] = -1; }
        for (int wg = 0; wg < w.grid; wg++) {
            int tm = -1, tn = -1;
            if (!x6_tile_of(w, wg, r, tm, tn)) continue;
            CHECK(r < w.rounds, "%s %d x %d: workgroup %d has a tile in round %d of %d", name, tiles_m, tiles_n, wg, r, w.rounds);
            if (tm < 0 || tm >= tiles_m || tn < 0 || tn >= tiles_n) { CHECK(false, "%s %d x %d: tile (%d, %d)", name, tiles_m, tiles_n, tm, tn); continue; }
            seen[tm * tiles_n + tn]++;
            const int x = wg & 7;
            if (tm < lo_m[x]) lo_m[x] = tm;
            if (tm > hi_m[x]) hi_m[x] = tm;
            if (tn < lo_n[x]) lo_n[x] = tn;
            if (tn > hi_n[x]) hi_n[x] = tn;
            if (w.rb == 0) {
                int om, on;
                old_tile_of(ntiles, tiles_n, wg + r * w.grid, om, on);
                CHECK(om == tm && on == tn, "%s %d x %d: row walk (%d, %d), the formula (%d, %d)", name, tiles_m, tiles_n, tm, tn, om, on);
            }
        }
        if (w.rb)
            for (int x = 0; x < 8; x++)
                CHECK(hi_m[x] < 0 || (hi_m[x] - lo_m[x] < w.rb && hi_n[x] - lo_n[x] < w.cb), "%s %d x %d: XCD %d round %d spans %d panels x %d column tiles",
                      name, tiles_m, tiles_n, x, r, hi_m[x] - lo_m[x] + 1, hi_n[x] - lo_n[x] + 1);
    }
    for (int t = 0; t < ntiles; t++) CHECK(seen[t] == 1, "%s %d x %d: tile %d visited %d times", name, tiles_m, tiles_n, t, seen[t]);
}

int main(int argc, char **argv) {
    if (argc > 1) {   // "query": the walk of one shape under the environment as it stands, through read_switches(); and what the kernel's
                      // tile loop meets on it: workgroups with no tile at all, workgroups that sit a round out and have a tile in a later
                      // one, tiles in blocks narrower than cb, tiles in blocks lower than rb
        const Switches sw = read_switches();
        const int tiles_m = atoi(argv[1]), tiles_n = atoi(argv[2]);
        const X6Walk w = x6_choose_walk(tiles_m, tiles_n, sw.x6_raster);
        int idle = 0, resume = 0, narrow = 0, low = 0;
        for (int wg = 0; wg < w.grid; wg++) {
            int tiles = 0, tm, tn;
            bool gap = false, resumed = false;
            for (int r = 0; r < w.rounds; r++) {
                if (!x6_tile_of(w, wg, r, tm, tn)) { gap = true; continue; }
                tiles++;
                if (gap) resumed = true;
                if (w.rb) {
                    narrow += tiles_n - tn / w.cb * w.cb < w.cb;
                    low += tiles_m - tm / w.rb * w.rb < w.rb;
                }
            }
            idle += tiles == 0;
            resume += resumed;
        }
        printf("%d %d %d %d %d %d %d %d\n", w.rb, w.cb, w.grid, w.rounds, idle, resume, narrow, low);
        return 0;
    }
    unsetenv("MDD_GEMM_X6_RASTER");
    const X6Raster dflt = read_switches().x6_raster;
    setenv("MDD_GEMM_X6_RASTER", "rows", 1);
    const X6Raster rows = read_switches().x6_raster;
    CHECK(rows.rb == 0, "MDD_GEMM_X6_RASTER=rows gives %d x %d", rows.rb, rows.cb);
    const struct { const char *env; int rb, cb; } parse[] = {{"2x16", 2, 16}, {"4x8", 4, 8}, {"8x4", 8, 4}, {"1x32", 1, 32},
        {"8x8", dflt.rb, dflt.cb}, {"0x8", dflt.rb, dflt.cb}, {"4x", dflt.rb, dflt.cb}, {"4x8x", dflt.rb, dflt.cb}, {"blocks", dflt.rb, dflt.cb}, {"", dflt.rb, dflt.cb}};
    for (const auto &p : parse) {
        const X6Raster got = x6_raster_from_env(p.env);
        CHECK(got.rb == p.rb && got.cb == p.cb, "\"%s\" parses to %d x %d", p.env, got.rb, got.cb);
    }
    // the strict parser the diagnostic entries use: a value is rows, a block shape of at most 32 tiles, or refused
    for (const char *ok : {"rows", "2x16", "4x8", "8x4", "1x32", "32x1"}) { X6Raster r; CHECK(x6_raster_parse(ok, &r), "\"%s\" refused", ok); }
    for (const char *no : {"row", "ROWS", "8x8", "0x8", "4x", "4x8x", "x8", "blocks", "", " 4x8 "}) {
        X6Raster r = {-1, -1};
        CHECK(!x6_raster_parse(no, &r) && r.rb == -1 && r.cb == -1, "\"%s\" accepted as %d x %d", no, r.rb, r.cb);
    }
    { X6Raster r; CHECK(!x6_raster_parse(nullptr, &r), "null accepted"); }
    CHECK(dflt.rb == 4 && dflt.cb == 8, "the default is %d x %d", dflt.rb, dflt.cb);
    const X6Raster arms[] = {dflt, rows, {4, 8}, {2, 16}, {8, 4}};
    const char *names[] = {"default", "rows", "4x8", "2x16", "8x4"};
    for (int a = 0; a < 5; a++)
        for (int tm = 1; tm <= 700; tm++)
            for (int tn = 1; tn <= 24; tn++) walk_shape(tm, tn, arms[a], names[a]);
    printf("default %d x %d; %d failure(s)\n", dflt.rb, dflt.cb, bad);
    return bad != 0;
}
'''


def _driver(tmp_path):
    src, exe = tmp_path / "raster_driver.cpp", str(tmp_path / "raster_driver")
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    return exe


def test_every_walk_visits_every_tile_once(tmp_path):
    """Panels 1..700 x column tiles 1..24 at grid 256, under the default, MDD_GEMM_X6_RASTER=rows and the 4x8 / 2x16 / 8x4 blocks: every tile
    exactly once and inside the matrix; a block walk's (XCD, round) within rb panels x cb column tiles; never more rounds than the row
    walk's ceil(ntiles / grid); the row walk exactly where the rule says (switch, tiles_n < cb, fewer than 32 tiles, more rounds); the row
    walk equal to the formula the kernel had, written out in the driver; and the switch's parser."""
    r = subprocess.run([_driver(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_walks_of_the_forward_s_own_launches(tmp_path):
    """The launches the decode forward makes at the headline shape, by name: 667 x 24 and 107 x 24 follow the default walk, 9 x 24 (one
    round in rows, two in 4 x 8 blocks) and the text table's 1 x 24 fall back, and the switch reaches the handle's Switches."""
    exe = _driver(tmp_path)

    def walk(tm, tn, raster=None):
        env = {k: v for k, v in os.environ.items() if k != "MDD_GEMM_X6_RASTER"}
        if raster:
            env["MDD_GEMM_X6_RASTER"] = raster
        return tuple(int(v) for v in subprocess.check_output([exe, str(tm), str(tn)], env=env, text=True).split())[:4]

    assert walk(667, 24, "4x8") == (4, 8, 256, 63)          # 167 x 3 = 501 blocks on 8 XCDs; the row walk: ceil(16008 / 256) = 63
    assert walk(107, 24, "4x8") == (4, 8, 256, 11)
    assert walk(9, 24, "4x8") == (0, 0, 216, 1)
    assert walk(1, 24, "4x8") == (0, 0, 24, 1)
    assert walk(667, 24, "8x4") == (8, 4, 256, 63)
    assert walk(667, 24, "2x16") == (0, 0, 256, 63)         # 24 column tiles are one and a half 16-wide blocks: 84 rounds, so rows
    assert walk(667, 32, "2x16") == (2, 16, 256, 84)
    assert walk(667, 24, "rows") == (0, 0, 256, 63)
    assert walk(667, 24) == (4, 8, 256, 63)                 # the default: what profiles/gemm_raster_notes.txt kept
    assert walk(667, 8, "2x16") == (0, 0, 256, 21)         # narrower than a block


def test_what_the_device_shapes_reach(tmp_path):
    """The shapes of tests/test_gemm_raster.py, by what the kernel's tile loop meets on each under the default walk: which walk the launcher
    takes, workgroups with no tile at all (the early return), workgroups that sit a round out and take a tile in a later one (tile_of's
    loop), tiles in blocks narrower than 8 and lower than 4.  The comments beside those shapes say this; here it is pinned."""
    from tests.test_gemm_raster import SHAPES
    exe = _driver(tmp_path)
    env = {k: v for k, v in os.environ.items() if k != "MDD_GEMM_X6_RASTER"}
    got = {}
    for M, N, K in SHAPES:
        tm, tn = (M + 191) // 192, (N + 127) // 128
        got[(M, N, K)] = tuple(int(v) for v in subprocess.check_output([exe, str(tm), str(tn)], env=env, text=True).split())
    # (rb, cb, grid, rounds, workgroups without a tile, workgroups resuming after a round sat out, tiles in narrow blocks, tiles in low blocks)
    want = {
        (6912, 1024, 32): (4, 8, 256, 2, 0, 0, 0, 0),
        (7877, 1152, 64): (0, 0, 256, 2, 0, 0, 0, 0),          # 22 blocks would be 3 rounds against 2: the row walk
        (7680, 1000, 96): (4, 8, 256, 2, 0, 0, 0, 0),
        (50000, 3072, 96): (4, 8, 256, 25, 0, 0, 0, 24),
        (1728, 3072, 64): (0, 0, 216, 1, 0, 0, 0, 0),
        (44, 3072, 512): (0, 0, 24, 1, 0, 0, 0, 0),
        (100, 64, 64): (0, 0, 1, 1, 0, 0, 0, 0),
        (1, 4, 32): (0, 0, 1, 1, 0, 0, 0, 0),
        (3072, 1920, 64): (4, 8, 256, 1, 16, 0, 112, 0),
        (4224, 1536, 64): (4, 8, 256, 2, 64, 0, 88, 24),       # XCDs 1, 3, 5, 7 only ever meet 4-wide blocks: 16 workgroups of each idle
        (6100, 2560, 64): (4, 8, 256, 3, 0, 80, 128, 0),        # five XCDs meet their 4-wide block before a full one: 16 workgroups of each resume
    }
    assert got == want
    assert any(v[0] and v[4] for v in got.values()) and any(v[0] and v[5] for v in got.values()) and any(v[0] and v[6] for v in got.values())
