"""What the MWER tests share (tests/test_ctc_nbest_grad_reference.py on the CPU, tests/test_ctc_nbest_grad.py and tests/test_mwer_loss.py
on the GPU, tools/time_ctc_nbest_grad.py): the float64 yardstick and csrc/plan.h's ctc_nbest_grad_plan itself, built with the host
compiler as tests/ctc_nbest_cases.py builds ctc_nbest_plan, so that no test restates the counts it takes from it.

The yardstick.  ``nll_f64`` is CPU ``torch.nn.functional.ctc_loss(reduction='none')`` on a double leaf tensor, one call per rank, as
tests/ctc_nbest_cases.reference makes it.  ``risk_f64`` puts the softmax over the ranks and the risk on top and calls autograd;
``weighted_grad_f64`` is the linear form ``sum_n coef[n,b] nll_n`` under autograd, so both give ATen's form of the gradient on the log-probs,
``exp(lp) - occupancy`` per rank.  A rank whose nll is +inf has posterior 0; autograd through it would give 0 * inf, so such ranks (and, in
the linear form, ranks with coef == 0) are left out of the graph -- which is what the kernel does with them.

Bounds.  GRAD_ATOL is the 5e-6 tests/ctc_loss_cases.py holds the wave forms of mdd_ctc_loss's gradient to: the output is a linear
combination of tensors each held to that bound, so |grad - f64| <= GRAD_ATOL * sum_n |coef[n,b]| per utterance.  CLASS_SUM (1e-4, same
file) bounds |sum over classes of a live frame| the same way."""
import collections
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests import ctc_loss_cases as lc
from tests import ctc_nbest_cases as cc

CSRC = cc.CSRC
GRAD_ATOL = lc.GRAD_ATOL["wave1"]
assert GRAD_ATOL == lc.GRAD_ATOL["wave2"] == lc.GRAD_ATOL["wave4"] == 5e-6
CLASS_SUM = lc.CLASS_SUM
LOGLIK_RTOL = cc.LOGLIK_RTOL
LDS_MAX = 160 * 1024

# `plan T B C N max_len`: one line of counts; no argument: the walk over shapes with the checks written out, then probes of the fits query
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
        const CtcNbestGradPlan p = ctc_nbest_grad_plan(T, B, C, N, max_len);
        printf("NL %d ranks %d groups %d SP %d smem %zu rows_bytes %zu slab_bytes %zu flag_bytes %zu bytes %zu fits %d\n", p.NL, p.ranks, p.groups, p.SP,
               p.smem, p.rows_bytes, p.slab_bytes, p.flag_bytes, p.bytes, (int)ctc_nbest_grad_fits(T, C, max_len));
        return 0;
    }
    size_t worst = 0;
    long accepted = 0;
    for (int C : {2, 3, 45, 101, 255, 256})
        for (int max_len : {0, 1, 63, 64, 127, 128, 254, 255})
            for (int T = 1; T <= 12000; T += (T < 500 ? 1 : 97)) {
                const int NL = max_len <= 63 ? 1 : max_len <= 127 ? 2 : 4;
                const size_t lds = ((size_t)8 * T * C + (size_t)2560 * NL + 4 * ((size_t)C + 1) + 15) / 16 * 16;
                if (!ctc_nbest_grad_fits(T, C, max_len)) { CHECK(lds > (size_t)160 * 1024 - 256, "T %d C %d max_len %d refused", T, C, max_len); continue; }
                accepted++;
                CHECK(ctc_nbest_fits(T, C, max_len), "T %d C %d max_len %d: accepted here, refused by ctc_nbest_fits", T, C, max_len);
                for (int N : {1, 2, 4, 5, 10, 11, 17, 100, 255, 256})
                    for (int B : {1, 2, 3, 32, 100, 256, 300, 65535}) {
                        const CtcNbestGradPlan p = ctc_nbest_grad_plan(T, B, C, N, max_len);
                        CHECK(p.NL == NL && p.NL == ctc_labels_per_lane(max_len) && 64 * p.NL >= max_len + 1, "max_len %d: NL %d", max_len, p.NL);
                        CHECK(p.smem == lds && p.smem <= (size_t)160 * 1024 && p.smem + 256 <= (size_t)160 * 1024, "T %d C %d: smem %zu", T, C, p.smem);
                        CHECK(p.ranks >= 1 && p.groups >= 1 && (long)p.groups * p.ranks >= N && (long)(p.groups - 1) * p.ranks < N, "N %d: %d groups of %d", N, p.groups, p.ranks);
                        CHECK((long)p.groups * B <= 256 || p.groups == 1, "N %d B %d: %d groups", N, B, p.groups);
                        CHECK(p.SP == 2 * (max_len + 1), "SP %d", p.SP);
                        const size_t rows = (size_t)8 * p.groups * B * 2 * T * p.SP, slabs = p.groups > 1 ? (size_t)4 * p.groups * T * B * C : 0,
                                     flags = p.groups > 1 ? (size_t)4 * p.groups * B : 0;
                        CHECK(p.rows_bytes == rows && p.slab_bytes == slabs && p.flag_bytes == flags && p.bytes == rows + slabs + flags, "T %d B %d C %d N %d: bytes %zu", T, B, C, N, p.bytes);
                        if (p.smem > worst) worst = p.smem;
                    }
            }
    CHECK(ctc_nbest_grad_fits(250, 45, 255), "the training shape is refused");
    CHECK(!ctc_nbest_grad_fits(0, 45, 64) && !ctc_nbest_grad_fits(40, 1, 64) && !ctc_nbest_grad_fits(40, 257, 64) && !ctc_nbest_grad_fits(40, 45, -1) &&
          !ctc_nbest_grad_fits(40, 45, 256) && ctc_nbest_grad_fits(1, 2, 0), "ctc_nbest_grad_fits' ranges");
    printf("accepted %ld shapes; largest LDS of a workgroup: %zu bytes; %ld mismatch(es)\n", accepted, worst, bad);
    for (int C : {2, 45, 256})
        for (int max_len : {10, 64, 255}) {
            int Tmax = 0;
            while (ctc_nbest_grad_fits(Tmax + 1, C, max_len)) Tmax++;
            printf("tmax %d %d %d\n", C, max_len, Tmax);
        }
    return bad != 0;
}
'''


@functools.lru_cache(maxsize=None)
def plan_driver():
    """Path of the built driver (csrc/plan.h with the host compiler), once per process."""
    d = tempfile.mkdtemp(prefix="ctc_nbest_grad_plan_")
    src, exe = os.path.join(d, "plan_driver.cpp"), os.path.join(d, "plan_driver")
    with open(src, "w") as f:
        f.write(PLAN_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


Plan = collections.namedtuple("Plan", "NL ranks groups SP smem rows_bytes slab_bytes flag_bytes bytes fits")


@functools.lru_cache(maxsize=None)
def plan(T, B, C, N, max_len):
    """ctc_nbest_grad_plan(T, B, C, N, max_len) and ctc_nbest_grad_fits(T, C, max_len) as csrc/plan.h computes them."""
    words = subprocess.run([plan_driver(), "plan", str(T), str(B), str(C), str(N), str(max_len)], capture_output=True, text=True, check=True).stdout.split()
    return Plan(**{k: int(v) for k, v in zip(words[0::2], words[1::2])})


def tmax(C, max_len):
    """The largest T ctc_nbest_grad_fits accepts at C classes and max_len ids (by the plan's own answers)."""
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if plan(mid, 1, C, 1, max_len).fits else (lo, mid - 1)
    return lo


# ----------------------------------------------------------------------------------------------------------------- float64
def _torch():
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return torch


def _rank_nll(x, lens, ids, nids, n, blank, max_len, zero_infinity=True):
    """nll [B] (double, on the graph of leaf ``x``) of rank n; lens and nids as the entries clamp them.  ``zero_infinity``: an infeasible
    row is 0 with a zero gradient (the graph builders mask such rows themselves), not +inf with a NaN one."""
    torch = _torch()
    T = x.shape[0]
    il = torch.from_numpy(np.clip(np.asarray(lens), 0, T).astype(np.int64))
    tl = torch.from_numpy(np.clip(np.asarray(nids[n]), 0, max_len).astype(np.int64))
    tg = torch.from_numpy(np.array(np.asarray(ids)[n, :, :max(max_len, 1)]).astype(np.int64))
    return torch.nn.functional.ctc_loss(x, tg, il, tl, blank=blank, reduction="none", zero_infinity=zero_infinity)


def nll_f64(lp, lens, ids, nids, blank=0, max_len=None):
    """nll [N, B] float64 (+inf where a hypothesis is no CTC path of the frames)."""
    torch = _torch()
    max_len = ids.shape[2] if max_len is None else max_len
    x = torch.from_numpy(np.array(lp)).double()
    with torch.no_grad():
        return np.stack([_rank_nll(x, lens, ids, nids, n, blank, max_len, zero_infinity=False).numpy() for n in range(ids.shape[0])])


def weighted_grad_f64(lp, lens, ids, nids, coef, blank=0, max_len=None):
    """[T, B, C] float64: what ``sum_{n,b} coef[n,b] nll_n[b]`` deposits on the log-probs (ATen's form per rank, frames >= len zeros);
    (n, b) pairs with coef == 0 are left out."""
    torch = _torch()
    max_len = ids.shape[2] if max_len is None else max_len
    coef = np.asarray(coef, dtype=np.float64)
    x = torch.from_numpy(np.array(lp)).double().requires_grad_(True)
    total = x.sum() * 0.0
    for n in range(ids.shape[0]):
        live = torch.from_numpy(coef[n] != 0)
        if bool(live.any()):
            nll = _rank_nll(x, lens, ids, nids, n, blank, max_len)
            total = total + (torch.from_numpy(coef[n])[live] * nll[live]).sum()
    total.backward()
    return x.grad.numpy()


Risk = collections.namedtuple("Risk", "nll post risk coef autograd_coef grad")


def risk_f64(lp, lens, ids, nids, cost, blank=0, max_len=None):
    """The MWER objective in float64: nll [N,B], post = softmax_n(-nll) [N,B], risk [B] = sum_n post cost, coef = post (risk - cost) (the
    closed form), autograd_coef = d risk_b / d nll_n as autograd finds it through the softmax, grad [T,B,C] = what sum_b risk_b deposits
    on the log-probs.  Ranks with nll = +inf have posterior 0 and are left out of the graph."""
    torch = _torch()
    max_len = ids.shape[2] if max_len is None else max_len
    N, B = ids.shape[:2]
    cost_t = torch.from_numpy(np.asarray(cost, dtype=np.float64))
    finite = torch.from_numpy(np.isfinite(nll_f64(lp, lens, ids, nids, blank, max_len)))
    assert bool(finite.any(dim=0).all()), "an utterance without a feasible hypothesis"
    x = torch.from_numpy(np.array(lp)).double().requires_grad_(True)
    rows = []
    for n in range(N):
        nll = _rank_nll(x, lens, ids, nids, n, blank, max_len)
        rows.append(torch.where(finite[n], nll, torch.zeros_like(nll).detach()))
    # the softmax over a leaf copy of the nll values, so that autograd's d risk / d nll can be read off before it goes on to the log-probs
    nll_graph = torch.stack(rows)
    nll_leaf = nll_graph.detach().clone().requires_grad_(True)
    ll = torch.where(finite, -nll_leaf, torch.full_like(nll_leaf, -float("inf")))
    post = torch.softmax(ll, dim=0)
    risk = (post * cost_t).sum(dim=0)
    risk.sum().backward()
    autograd_coef = torch.where(finite, nll_leaf.grad, torch.zeros_like(nll_leaf))
    live = finite & (autograd_coef != 0)
    (autograd_coef[live] * nll_graph[live]).sum().backward()
    post_n, risk_n = post.detach().numpy(), risk.detach().numpy()
    nll_n = np.where(finite.numpy(), nll_leaf.detach().numpy(), np.inf)
    return Risk(nll_n, post_n, risk_n, post_n * (risk_n[None, :] - cost_t.numpy()), autograd_coef.numpy(), x.grad.numpy())


def utterance_bounds(coef):
    """(GRAD_ATOL sum_n |coef[n,b]|, CLASS_SUM sum_n |coef[n,b]|) per utterance."""
    s = np.abs(np.asarray(coef, dtype=np.float64)).sum(axis=0)
    return GRAD_ATOL * s, CLASS_SUM * s


# ------------------------------------------------------------------------------------------------------------------- inputs
def no_repeat_lists(seed, N, B, C, blank, longest, pitch):
    """ids [N,B,pitch] / nids [N,B]: hypotheses without adjacent repeats or the blank, so that each is a CTC path of ``its length``
    frames; rank 0 of utterance 0 has exactly ``longest`` ids, the others between longest // 2 and longest."""
    rs = np.random.default_rng(seed)
    classes = np.array([c for c in range(C) if c != blank])
    ids, nids = np.zeros((N, B, pitch), dtype=np.int32), np.zeros((N, B), dtype=np.int32)
    for n in range(N):
        for b in range(B):
            L = longest if (n, b) == (0, 0) else int(rs.integers(longest // 2, longest + 1))
            seq = [int(rs.integers(len(classes)))]
            while len(seq) < L:
                k = int(rs.integers(len(classes)))
                if k != seq[-1]:
                    seq.append(k)
            ids[n, b, :L], nids[n, b] = classes[np.array(seq[:L], dtype=np.int64)], L
    return ids, nids


def draw_coef(seed, N, B):
    """Coefficients of both signs, |coef| in [0.05, 1], not summing to zero: the exp(lp) * sum coef term is on trial too."""
    rs = np.random.default_rng(seed)
    return rs.uniform(0.05, 1.0, size=(N, B)) * rs.choice([-1.0, 1.0], size=(N, B))
