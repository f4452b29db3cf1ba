"""csrc/plan.h with the host compiler: beam_plan, everything the beam entries decide from numbers, against the expressions written out.

mdd_beam and mdd_beam_nbest take their prefix-row width, the generic kernel's LDS need and whether the LM table is in it, the route, the
single-wave kernel's instantiation and LDS terms, the waves per workgroup and the refusal (with the byte count its message prints) from
one pure function.  The driver restates each as the host function computed it before the plan existed and compares over every beam
1..64, every C 2..256, T 1..4200 (every value up to 700, every 7th beyond) and both entries.  That whole grid is walked once for each of
the fourteen switch settings -- MDD_BEAM_W unset and 0..5, MDD_BEAM_GENERIC on and off -- the switches going through the environment and
read_beam_switches() as they do in a call.  B enters the waves per workgroup alone, which only a shape with beam <= 16 and C <= 64 can
have: those shapes are walked at B in {1, 64, 65, 130, 512}, the others at B = 65.  It also prints the longest T the plan accepts at the two shapes include/mdd_hip.h names."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")

_DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include "plan.h"
using namespace mdd;

// What the host function of the beam entries computed, written out: no call into plan.h, no constant of it.
struct Old { int Tcap, lm_in_lds, fast, NS, W, refusal; size_t base, smem, pw, lmb, bytes; };   // refusal 0 none, 1 generic LDS, 2 single-wave LDS
static Old old_dispatch(int T, int B, int C, int beam, bool generic_env, const char *we) {
    Old o = {};
    const int FB = 16;
    o.Tcap = (T + 1 + 3) & ~3;
    const size_t lm_bytes = sizeof(double) * (size_t)(C + 1) * (C + 1);
    o.base = (sizeof(double) * 2 + sizeof(int)) * (size_t)beam * C + (size_t)(2 * beam + 1) * o.Tcap;
    o.lm_in_lds = (o.base + lm_bytes <= 96 * 1024) ? 1 : 0;
    o.smem = o.base + (o.lm_in_lds ? lm_bytes : 0);
    if (o.smem > 140 * 1024) { o.refusal = 1; o.bytes = o.smem; return o; }
    const int nslots = beam * C;
    o.fast = beam <= FB && C <= 64 && nslots <= 1024 && !generic_env;
    o.NS = nslots <= 512 ? 8 : 16;
    o.lmb = (sizeof(double) * (size_t)(C + 1) * (C + 1) + 15) & ~(size_t)15;
    const size_t wave = sizeof(double) * ((size_t)2 * o.NS * 64 + 64 + 6 * FB + 4 * FB) + sizeof(unsigned long long) * 4 * FB +
                        sizeof(int) * ((size_t)2 * o.NS * 64 + 4 * FB + 2 * FB) + (size_t)(2 * FB + 1) * o.Tcap;
    o.pw = (wave + 15) & ~(size_t)15;
    const size_t lds_max = 160 * 1024;
    if (o.fast && o.lmb + o.pw > lds_max) { o.refusal = 2; o.bytes = o.lmb + o.pw; return o; }
    if (o.fast) {
        int W = (int)((lds_max - o.lmb) / o.pw);
        W = W > 4 ? 4 : W;
        if (B <= 64) W = 1;
        if (we) { const int w = atoi(we); if (w >= 1 && w <= W) W = w; }
        o.W = W;
    }
    return o;
}

static long bad = 0, compared = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static void compare(int T, int B, int C, int beam, bool nb, bool generic_env, const char *we, const BeamSwitches &sw) {
    const Old o = old_dispatch(T, B, C, beam, generic_env, we);
    const BeamPlan p = beam_plan(T, B, C, beam, nb, sw);
    compared++;
    const int refusal = p.over == BeamLimit::Ok ? 0 : p.over == BeamLimit::GenericLds ? 1 : 2;
#define WHERE "T %d B %d C %d beam %d nbest %d generic %d W=%s: "
#define ARGS T, B, C, beam, (int)nb, (int)generic_env, we ? we : "(unset)"
    CHECK(p.nbest == nb, WHERE "nbest %d", ARGS, (int)p.nbest);
    CHECK(refusal == o.refusal, WHERE "refusal %d, written out %d", ARGS, refusal, o.refusal);
    CHECK(p.Tcap == o.Tcap && p.lm_in_lds == o.lm_in_lds && p.smem == o.smem, WHERE "Tcap %d lm_in_lds %d smem %zu, written out %d %d %zu", ARGS,
          p.Tcap, p.lm_in_lds, p.smem, o.Tcap, o.lm_in_lds, o.smem);
    CHECK(p.smem == o.base + (o.lm_in_lds ? 8 * (size_t)(C + 1) * (C + 1) : 0), WHERE "smem %zu against base %zu", ARGS, p.smem, o.base);
    if (o.refusal) CHECK(p.over_bytes == o.bytes, WHERE "message bytes %zu, written out %zu", ARGS, p.over_bytes, o.bytes);
    if (o.refusal == 1) return;
    CHECK((int)p.fast == o.fast && p.NS == o.NS && p.lmb == o.lmb && p.pw == o.pw, WHERE "fast %d NS %d lmb %zu pw %zu, written out %d %d %zu %zu", ARGS,
          (int)p.fast, p.NS, p.lmb, p.pw, o.fast, o.NS, o.lmb, o.pw);
    if (o.refusal) return;
    CHECK(p.W == o.W && (p.W >= 1) == p.fast, WHERE "W %d, written out %d", ARGS, p.W, o.W);
}

static int max_T(int beam, int C) {
    int best = 0;
    for (int T = 1; T <= 6000; T++) if (beam_plan(T, 1, C, beam, false, BeamSwitches()).over == BeamLimit::Ok) best = T;
    return best;
}

int main() {
    const char *ws[] = {nullptr, "0", "1", "2", "3", "4", "5"};
    const int Bs[] = {1, 64, 65, 130, 512};
    for (int g = 0; g < 2; g++)
        for (const char *we : ws) {
            if (g) setenv("MDD_BEAM_GENERIC", "1", 1); else unsetenv("MDD_BEAM_GENERIC");
            if (we) setenv("MDD_BEAM_W", we, 1); else unsetenv("MDD_BEAM_W");
            const BeamSwitches sw = read_beam_switches();   // per call, as the entries read them
            CHECK(sw.generic == (g != 0) && sw.w == (we ? atoi(we) : 0), "switches read as generic %d w %d", (int)sw.generic, sw.w);
            for (int beam = 1; beam <= 64; beam++)
                for (int C = 2; C <= 256; C++)
                    for (int T = 1; T <= 4200; T += T < 700 ? 1 : 7)
                        for (int nb = 0; nb < 2; nb++) {
                            const bool wide = beam <= 16 && C <= 64;   // B matters to W alone
                            for (int bi = 0; bi < (wide ? 5 : 1); bi++) compare(T, Bs[wide ? bi : 2], C, beam, nb != 0, g != 0, we, sw);
                        }
        }
    unsetenv("MDD_BEAM_GENERIC");
    unsetenv("MDD_BEAM_W");
    printf("max T: beam 10 C 45 -> %d; beam 64 C 45 -> %d\n", max_T(10, 45), max_T(64, 45));
    printf("%ld comparisons; %ld mismatch(es)\n", compared, bad);
    return bad != 0;
}
'''


def test_beam_plan_equals_the_expressions_written_out(tmp_path):
    """Zero mismatches over the grid of the module docstring; and the longest accepted T at (beam 10, C 45) and (beam 64, C 45) are the
    3995 and 663 include/mdd_hip.h states (tests/test_decoders.py derives the same two from its Python restatement alone)."""
    src, exe = tmp_path / "beam_plan_driver.cpp", str(tmp_path / "beam_plan_driver")
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDD_BEAM_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "; 0 mismatch(es)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"max T: beam 10 C 45 -> (\d+); beam 64 C 45 -> (\d+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (3995, 663), r.stdout[-500:]
    assert int(re.search(r"(\d+) comparisons", r.stdout).group(1)) > 600_000_000   # fourteen switch settings x the whole grid
