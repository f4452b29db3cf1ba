"""csrc/gemm_raster.h with the host compiler: x6_choose_tile, the rule that gives a launch of gemm_f32x6_kernel its tile -- 256 x 128
(RT = 4) or 192 x 128 (RT = 3) -- and that tile's walk.

For every launch of 1..700 row panels of 192 x 1..24 column tiles (at a row count that fills its last 192-row panel, at one that holds a
single row of it, and at the same counts of 256-row panels) the rule names an instantiation the library has, by the rule's own statement
4 x rounds(RT = 4) <= 3 x rounds(RT = 3); and the walk it returns is that instantiation's own: every tile of its tile counts taken exactly
once, inside the matrix.  The forward's own launches are pinned by name."""
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

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static void every_tile_once(const X6Tile &t, int M, int tiles_n, const char *name) {
    const int tiles_m = (M + 64 * t.rt - 1) / (64 * t.rt), ntiles = tiles_m * tiles_n;
    const X6Walk &w = t.walk;
    CHECK(w.ntiles == ntiles && w.tiles_n == tiles_n, "%s M %d x %d: RT %d, walk of %d tiles (%d wide), the launch has %d", name, M, tiles_n, t.rt, w.ntiles, w.tiles_n, ntiles);
    CHECK(w.grid >= 1 && w.grid <= 256 && w.rounds >= 1, "%s M %d x %d: grid %d rounds %d", name, M, tiles_n, w.grid, w.rounds);
    std::vector<int> seen(ntiles, 0);
    for (int r = 0; r <= w.rounds; r++)
        for (int wg = 0; wg < w.grid; wg++) {
            int tm = -1, tn = -1;
            if (!x6_tile_of(w, wg, r, tm, tn)) continue;
            CHECK(r < w.rounds, "%s M %d x %d: a tile in round %d of %d", name, M, tiles_n, r, w.rounds);
            if (tm < 0 || tm >= tiles_m || tn < 0 || tn >= tiles_n) { CHECK(false, "%s M %d x %d: tile (%d, %d)", name, M, tiles_n, tm, tn); continue; }
            CHECK(tm * 64 * t.rt < M, "%s M %d x %d: panel %d starts past the last row", name, M, tiles_n, tm);
            seen[tm * tiles_n + tn]++;
        }
    for (int i = 0; i < ntiles; i++) CHECK(seen[i] == 1, "%s M %d x %d: RT %d tile %d visited %d times", name, M, tiles_n, t.rt, i, seen[i]);
}

static void one(int M, int tiles_n, X6Raster want, const char *name, long long *taken4) {
    const X6Tile t = x6_choose_tile(M, tiles_n, want);
    CHECK(t.rt == 3 || t.rt == 4, "%s M %d x %d: RT %d", name, M, tiles_n, t.rt);
    const X6Walk w3 = x6_choose_walk((M + 191) / 192, tiles_n, want), w4 = x6_choose_walk((M + 255) / 256, tiles_n, want);
    CHECK(t.rt == (4 * w4.rounds <= 3 * w3.rounds ? 4 : 3), "%s M %d x %d: RT %d at %d rounds of 256 rows against %d of 192", name, M, tiles_n, t.rt, w4.rounds, w3.rounds);
    CHECK(t.rt == 3 || w3.rounds >= 2, "%s M %d x %d: RT 4 in a launch that 192-row tiles finish in one round", name, M, tiles_n);
    *taken4 += t.rt == 4;
    every_tile_once(t, M, tiles_n, name);
    for (int rt = 3; rt <= 4; rt++) {   // the switch's forced tiles
        const X6Tile f = x6_choose_tile(M, tiles_n, want, rt);
        CHECK(f.rt == rt, "%s M %d x %d: forced RT %d gives %d", name, M, tiles_n, rt, f.rt);
        every_tile_once(f, M, tiles_n, name);
    }
}

int main(int argc, char **argv) {
    if (argc > 1) {   // "query": rows, column tiles -> the tile and walk under the environment as it stands, through read_switches()
        const Switches sw = read_switches();
        const X6Tile t = x6_choose_tile(atoi(argv[1]), atoi(argv[2]), sw.x6_raster, sw.x6_rt);
        printf("%d %d %d %d %d\n", t.rt, t.walk.rb, t.walk.cb, t.walk.grid, t.walk.rounds);
        return 0;
    }
    for (const char *ok : {"3", "4"}) { int rt = -1; CHECK(x6_rt_parse(ok, &rt) && rt == ok[0] - '0' && x6_rt_from_env(ok) == rt, "\"%s\" refused", ok); }
    for (const char *no : {"", "2", "5", "34", "4 ", " 4", "four", "3.0"}) {
        int rt = -1;
        CHECK(!x6_rt_parse(no, &rt) && rt == -1 && x6_rt_from_env(no) == kX6RtRule, "\"%s\" accepted as %d", no, rt);
    }
    { int rt; CHECK(!x6_rt_parse(nullptr, &rt) && x6_rt_from_env(nullptr) == kX6RtRule, "null accepted"); }
    const X6Raster arms[] = {kX6DefaultRaster, kX6Rows, {8, 4}};
    const char *names[] = {"default", "rows", "8x4"};
    long long taken4 = 0, launches = 0;
    for (int a = 0; a < 3; a++)
        for (int tm = 1; tm <= 700; tm++)
            for (int tn = 1; tn <= 24; tn++) {
                one(tm * 192, tn, arms[a], names[a], &taken4);
                one(tm * 192 - 191, tn, arms[a], names[a], &taken4);
                if (tm * 256 <= 700 * 192) one(tm * 256, tn, arms[a], names[a], &taken4);
                launches += 2 + (tm * 256 <= 700 * 192);
            }
    CHECK(taken4 > launches / 4 && taken4 < launches, "RT 4 in %lld of %lld launches", taken4, launches);
    printf("RT 4 in %lld of %lld launches; %d failure(s)\n", taken4, launches, bad);
    return bad != 0;
}
'''


def _driver(tmp_path):
    src, exe = tmp_path / "rule_driver.cpp", str(tmp_path / "rule_driver")
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    return exe


def test_rule_names_an_instantiation_and_its_walk_visits_every_tile_once(tmp_path):
    r = subprocess.run([_driver(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_tiles_of_the_forward_s_own_launches(tmp_path):
    """By name: the headline's 128000 rows (500 panels of 256: 47 rounds against 63), --fuse 1's 16000 and --fuse 3's 48000 take RT = 4
    (6 against 8 and 18 against 24 rounds: the same MFMA time in fewer, fuller K-tiles); the text table's 44 rows, a 300-row
    projection and anything of one round stay on RT = 3; and the switch reaches the handle's Switches."""
    exe = _driver(tmp_path)

    def tile(M, tn, rt=None):
        env = {k: v for k, v in os.environ.items() if k not in ("MDD_GEMM_X6_RASTER", "MDD_GEMM_X6_RT")}
        if rt:
            env["MDD_GEMM_X6_RT"] = rt
        return tuple(int(v) for v in subprocess.check_output([exe, str(M), str(tn)], env=env, text=True).split())

    assert tile(128000, 24) == (4, 4, 8, 256, 47)
    assert tile(128000, 24, "3") == (3, 4, 8, 256, 63)
    assert tile(16000, 24) == (4, 4, 8, 256, 6)
    assert tile(16000, 24, "3") == (3, 4, 8, 256, 8)
    assert tile(48000, 24) == (4, 4, 8, 256, 18)
    assert tile(48000, 24, "3") == (3, 4, 8, 256, 24)
    assert tile(44, 24) == (3, 0, 0, 24, 1)
    assert tile(44, 24, "4") == (4, 0, 0, 24, 1)
    assert tile(300, 24) == (3, 4, 8, 256, 1)
    assert tile(300, 24, "4") == (4, 4, 8, 256, 1)
    assert tile(300, 24, "five") == (3, 4, 8, 256, 1)       # at create any other value is the default: the rule
