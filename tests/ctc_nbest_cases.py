"""Inputs for mdd_ctc_nbest (csrc/ctc_nbest.hip), shared by tests/test_ctc_nbest_reference.py (CPU), tests/test_ctc_nbest.py (GPU) and
tools/time_ctc_nbest.py: posteriors (``synth.peaky_logp`` as tests/test_nbest.py stacks it, and random dense log-softmax rows), N-best lists
(per utterance a base sequence and 0-3 edits per rank, ``tests/mbr_reference.edited``; no label is the blank, as a beam's hypotheses have
none), the float64 yardstick (CPU ``torch.nn.functional.ctc_loss`` on a double tensor, as tests/ctc_loss_cases.py calls it), and
``plan``: csrc/plan.h's ctc_nbest_plan itself, built with the host compiler, so that no test restates the counts it takes from it.

Every array of a case is made once and shared, read-only."""
import collections
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests import mbr_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")
LOGLIK_RTOL = 1e-6          # the bound tests/test_nbest.py holds the per-rank loop to
MAX_LEN = 255               # include/mdd_hip.h: mdd_ctc_nbest's bound on max_len
MAX_N = 256

Case = collections.namedtuple("Case", "name lp lens ids nids blank max_len")

# What csrc/plan.h says, printed: `plan T B C N max_len` one line of counts; `walk` the checks of the plan against the expressions
# written out, then one line per probed (T, C, max_len) with ctc_nbest_fits' answer for the library to be compared with.
PLAN_DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "plan.h"
using namespace mdd;

static long bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const int T = atoi(argv[2]), B = atoi(argv[3]), C = atoi(argv[4]), N = atoi(argv[5]), max_len = atoi(argv[6]);
        const CtcNbestPlan p = ctc_nbest_plan(T, B, C, N, max_len, read_ctc_nbest_switches());
        printf("waves %d hyps_per_block %d NL %d smem %zu groups %d fits %d\n", p.waves, p.hyps_per_block, p.NL, p.smem, p.groups,
               (int)ctc_nbest_fits(T, C, max_len));
        return 0;
    }
    size_t worst = 0;
    long accepted = 0;
    for (int C : {2, 3, 45, 101, 255, 256})
        for (int max_len : {0, 1, 2, 63, 64, 65, 127, 128, 129, 254, 255})
            for (int T = 1; T <= 20000; T += (T < 800 ? 1 : 97)) {
                if (!ctc_nbest_fits(T, C, max_len)) { CHECK((size_t)4 * T * C > (size_t)116 * 1024, "T %d C %d max_len %d refused", T, C, max_len); continue; }
                accepted++;
                for (int N : {1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 35, 199, 200, 255, 256})
                    for (int h : {0, 1, 3, 8, 64, 256}) {
                        CtcNbestSwitches sw;
                        sw.hpb = h;
                        sw.waves = h % 5;
                        const int B = h == 0 ? (T % 2 ? 3 : 64) : (T % 2 ? 1 : 512);
                        const CtcNbestPlan p = ctc_nbest_plan(T, B, C, N, max_len, sw);
                        if (h == 0) {       // the rule written out: four ranks a workgroup while every scan can have a SIMD of its own, ten beyond, dealt evenly
                            const bool spread = 2 * (size_t)4 * T * C <= (size_t)160 * 1024 && N * B <= 1024;
                            const int target = spread ? 4 : 10, groups = (N + target - 1) / target;
                            CHECK(p.hyps_per_block == (N + groups - 1) / groups && p.groups == groups && p.waves == 8, "T %d B %d C %d N %d: %d ranks x %d groups", T, B, C, N, p.hyps_per_block, p.groups);
                        }
                        const int NL = max_len <= 63 ? 1 : max_len <= 127 ? 2 : 4;
                        CHECK(p.NL == NL && p.NL == ctc_labels_per_lane(max_len) && 64 * p.NL >= max_len + 1, "T %d C %d max_len %d: NL %d", T, C, max_len, p.NL);
                        CHECK(p.smem == (size_t)4 * T * C && p.smem <= (size_t)160 * 1024 && p.smem <= kCtcNbestLdsMax, "T %d C %d: smem %zu", T, C, p.smem);
                        CHECK(p.waves >= 1 && p.waves <= 16 && (sw.waves == 0 || p.waves == sw.waves) && p.hyps_per_block >= 1 && (h == 0 || p.hyps_per_block == h), "waves %d hyps_per_block %d (switch %d)", p.waves, p.hyps_per_block, h);
                        CHECK((long)p.groups * p.hyps_per_block >= N && (long)(p.groups - 1) * p.hyps_per_block < N && p.groups >= 1, "N %d: groups %d of %d", N, p.groups, p.hyps_per_block);
                        if (p.smem > worst) worst = p.smem;
                    }
            }
    CHECK(!ctc_nbest_fits(0, 45, 64) && !ctc_nbest_fits(40, 1, 64) && !ctc_nbest_fits(40, 257, 64) && !ctc_nbest_fits(40, 45, -1) &&
          !ctc_nbest_fits(40, 45, 256) && ctc_nbest_fits(1, 2, 0) && ctc_nbest_fits(116, 256, 255), "ctc_nbest_fits' ranges");
    printf("accepted %ld shapes; largest LDS of a workgroup: %zu bytes; %ld mismatch(es)\n", accepted, worst, bad);
    for (int C : {2, 45, 256}) {
        int Tmax = 0;
        while (ctc_nbest_fits(Tmax + 1, C, 64)) Tmax++;
        printf("tmax %d %d\n", C, Tmax);
        for (int max_len : {-1, 0, 64, 255, 256})
            for (int T : {0, 1, 116, 117, 659, 660, Tmax - 1, Tmax, Tmax + 1, Tmax + 100})
                printf("fits %d %d %d %d\n", T, C, max_len, (int)ctc_nbest_fits(T, C, max_len));
    }
    return bad != 0;
}
'''


@functools.lru_cache(maxsize=None)
def plan_driver():
    """Path of the built driver (csrc/plan.h with the host compiler), once per process."""
    d = tempfile.mkdtemp(prefix="ctc_nbest_plan_")
    src, exe = os.path.join(d, "plan_driver.cpp"), os.path.join(d, "plan_driver")
    with open(src, "w") as f:
        f.write(PLAN_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


Plan = collections.namedtuple("Plan", "waves hyps_per_block NL smem groups fits")


@functools.lru_cache(maxsize=None)
def plan(T, B, C, N, max_len):
    """ctc_nbest_plan(T, B, C, N, max_len) and ctc_nbest_fits(T, C, max_len) as csrc/plan.h computes them (without the sweep's switches)."""
    env = {k: v for k, v in os.environ.items() if k not in ("MDD_CTC_NBEST_HPB", "MDD_CTC_NBEST_WAVES")}
    words = subprocess.run([plan_driver(), "plan", str(T), str(B), str(C), str(N), str(max_len)], capture_output=True, text=True, check=True, env=env).stdout.split()
    return Plan(**{k: int(v) for k, v in zip(words[0::2], words[1::2])})


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def dense_logp(seed, T, B, C, scale=2.0):
    """Random dense log-softmax rows [T, B, C] fp32 (tests/ctc_loss_cases.py's)."""
    rs = np.random.Generator(np.random.PCG64(seed))
    z = rs.standard_normal((T, B, C)) * scale
    z = z - z.max(axis=-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=-1, keepdims=True))).astype(np.float32)


def peaky_logp(seed, T, B, C):
    """tests/test_nbest.py's stack of synth.peaky_logp utterances (the blank boosted is class 0)."""
    from ctc_attention_mispronunciation_amd import synth
    return np.stack([synth.peaky_logp(T, C, max(1, T // 8) + b, seed=seed + b) for b in range(B)], axis=1)


def draw_lists(seed, N, B, C, blank, lo, hi, pitch, max_len=None):
    """(ids [N,B,pitch] int32, nids [N,B] int32): per utterance a base sequence of lo..hi labels (for utterance b: lo[b]..hi[b] where
    sequences are given) without the blank, which is rank 0; per further rank 0-3 random edits of it cut to ``max_len`` (default hi).
    Behind a row's length the ids are 0."""
    rs = np.random.default_rng(seed)
    classes = np.array([c for c in range(C) if c != blank])
    ids, nids = np.zeros((N, B, pitch), dtype=np.int32), np.zeros((N, B), dtype=np.int32)
    for b in range(B):
        lo_b, hi_b = (lo[b], hi[b]) if isinstance(lo, (tuple, list)) else (lo, hi)
        cap = hi_b if max_len is None else max_len
        base = rs.integers(0, C - 1, size=int(rs.integers(lo_b, hi_b + 1))).tolist()
        for n in range(N):
            seq = mr.edited(rs, base, C - 1, cap, int(rs.integers(0, 4)) if n else 0)      # rank 0 is the base itself
            ids[n, b, :len(seq)], nids[n, b] = classes[np.array(seq, dtype=np.int64)], len(seq)
    return ids, nids


_CASES = {}


def make(name, lp, lens, ids, nids, blank, max_len):
    """A case under its name (``reference`` looks it up by that)."""
    lens, nids = np.asarray(lens, dtype=np.int32), np.asarray(nids, dtype=np.int32)
    _CASES[name] = Case(name, *_frozen(lp, lens, ids, nids), blank, max_len)
    return _CASES[name]


RAGGED = (40, 33, 21)       # lens of the T = 40 cases, repeated over the batch: every one >= 2 * 10 + 1, the longest row


@functools.lru_cache(maxsize=None)
def ragged(kind, C=45, blank=0, N=MAX_N, seed=0, B=3):
    """T = 40, lens RAGGED (B = 3; repeated for more), rows of at most 10 ids, N = 256 ranks (a test takes the first N it needs).  At
    B = 3 no list has more scans than the device has SIMDs, at B = 6 the longer ones do: the two branches of the plan's rule."""
    lp = peaky_logp(2100 + seed, 40, B, C) if kind == "peaky" else dense_logp(2200 + seed, 40, B, C)
    if kind == "peaky" and blank != 0:           # the boosted class to where the blank is
        lp = lp.copy()
        lp[:, :, [0, blank]] = lp[:, :, [blank, 0]]
    ids, nids = draw_lists(2300 + seed + C + blank, N, B, C, blank, 5, 8, pitch=40, max_len=10)
    return make("ragged_%s_C%d_blank%d_B%d" % (kind, C, blank, B), lp, (RAGGED * B)[:B], ids, nids, blank, 10)


@functools.lru_cache(maxsize=None)
def form(longest):
    """B = 2, N = 3, T = 300, C = 45; max_len = longest, and rank 0 of utterance 0 has exactly that many ids: where the scan changes its
    labels per lane (63 | 64, 127 | 128) and its last label count (255).  Utterance 1 is ragged (len 280, shorter rows)."""
    T, B, N, C = 300, 2, 3, 45
    lp = dense_logp(2400 + longest, T, B, C)
    ids, nids = draw_lists(2500 + longest, N, B, C, 0, (longest, max(1, longest // 2)), (longest, max(1, longest // 2 + 9)), pitch=T, max_len=longest)
    return make("form_L%d" % longest, lp, (T, 280), ids, nids, 0, longest)


@functools.lru_cache(maxsize=None)
def bound(C, T, N):
    """B = 1 at a given T (the largest one mdd_ctc_nbest_fits accepts at C, in the test that asks), rows of 8..14 ids."""
    lp = dense_logp(2600 + C, T, 1, C)
    ids, nids = draw_lists(2700 + C, N, 1, C, 0, 8, 12, pitch=16, max_len=14)
    return make("bound_C%d_T%d" % (C, T), lp, (T,), ids, nids, 0, 14)


@functools.lru_cache(maxsize=None)
def reference(name, N=None):
    """float64 log-likelihoods [N, B] of the first N ranks of the case of that name: CPU torch.nn.functional.ctc_loss on a double tensor, reduction 'none',
    negated; -inf where it finds no path.  lens and nids as the entry clamps them."""
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(min(16, torch.get_num_threads()))
    case = _CASES[name]
    N = case.ids.shape[0] if N is None else N
    T = case.lp.shape[0]
    x = torch.from_numpy(np.array(case.lp)).double()
    il = torch.from_numpy(np.clip(case.lens, 0, T).astype(np.int64))
    out = np.empty((N, case.lp.shape[1]), dtype=np.float64)
    for n in range(N):
        tl = torch.from_numpy(np.clip(case.nids[n], 0, case.max_len).astype(np.int64))
        tg = torch.from_numpy(np.array(case.ids[n, :, :max(case.max_len, 1)]).astype(np.int64))
        out[n] = -F.ctc_loss(x, tg, il, tl, blank=case.blank, reduction="none").numpy()
    out.setflags(write=False)
    return out


def loglik_rel_err(got, ref):
    """Worst |got - ref| / |ref| where the reference is finite; where it is -inf, got must be."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert (got[~fin] == ref[~fin]).all(), (got[~fin], ref[~fin])
    return float((np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])).max(initial=0.0))
