#!/usr/bin/env python3
"""What the minimum-Bayes-risk decode of an N-best list costs: mdd_nbest_mbr (all N x N edit distances of every utterance, the risks, the
argmin; csrc/mbr.hip) at four shapes (B, N, max_len) = (64, 10, 64), (64, 200, 64), (512, 10, 64), (64, 200, 256), beside three things
a caller would compare it with:

  host      mdd_align_batch (csrc/host_align.cpp: the full-matrix DP with backtrace, the only way the tree computed an edit distance before
            the entry existed) over the same B N^2 pairs, one thread.  Timed on a sample of --host_pairs pairs drawn evenly from them (an
            empty side is replaced by one id: the host entry refuses it) and scaled to the whole count; the notes say how many were timed.
  rescore   BeamDecoder.nbest_loglik on the same list: one mdd_ctc_loss without gradient per rank, ending in the copy to the host.
  search    the beam search that makes such a list: mdd_beam_nbest, or mdd_beam_wide where mdd_beam_fits says so, at beam = nbest = N.

The lists are what an N-best list looks like: per utterance a random base sequence of max_len / 2 .. max_len ids, per hypothesis 0-3
random edits of it (tests/mbr_reference.draw_lists); weights a softmax of random log-likelihoods; C = 45; a reference row per utterance,
dist / ref_dist / ref_risk all asked for.  The posteriors of `rescore` and `search` are peaky ones (synth.peaky_logp) of T = 250 frames
(T = 600 at max_len 256).  Every GPU call is timed on its own between two HIP events after --warmup untimed calls, back to back; the
figure is the median of --reps >= 20 calls with the minimum and maximum beside it.  The entry's call includes its three launches and
its workspace from torch's allocator (hip_model.nbest_mbr).  One JSON line per run; --out writes the notes file as well.

Usage:  python tools/time_mbr.py [--reps 30] [--warmup 5] [--host_pairs 20000] [--out profiles/mbr_notes.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CN = 45
SHAPES = ((64, 10, 64), (64, 200, 64), (512, 10, 64), (64, 200, 256))


def timed(fn, reps, warmup, sync_each=False):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
        if sync_each:
            e1.synchronize()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def host_align(ids, nids, pairs):
    """Seconds mdd_align_batch takes for `pairs` (b, n, m) triples of the list, one call, one thread."""
    import numpy as np
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import align_ids_batch
    b, n, m = pairs.T
    a, al = ids[n, b].copy(), np.maximum(nids[n, b], 1)
    t, tl = ids[m, b].copy(), np.maximum(nids[m, b], 1)
    align_ids_batch(a[:64], al[:64], t[:64], tl[:64])
    t0 = time.perf_counter()
    align_ids_batch(a, al, t, tl)
    return time.perf_counter() - t0


def run(B, N, max_len, reps, warmup, host_pairs):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import _lib, synth
    from ctc_attention_mispronunciation_amd.hip_model import nbest_mbr
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from tests import mbr_reference as mr
    ids_h, nids_h = mr.draw_lists(4000 + B + N + max_len, N, B, CN, max_len, pitch=max_len)
    ref_h, ref_len_h = mr.draw_lists(5000 + B + N + max_len, 1, B, CN, max_len, pitch=max_len)
    w_h = mr.softmax_weights(6000 + B + N, N, B)
    ids, nids, w = torch.from_numpy(ids_h).cuda(), torch.from_numpy(nids_h).cuda(), torch.from_numpy(w_h).cuda()
    ref, ref_len = torch.from_numpy(ref_h[0]).cuda(), torch.from_numpy(ref_len_h[0]).cuda()
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    res = dict(B=B, N=N, max_len=max_len, pairs=B * N * N, mean_len=float(nids_h.mean()))

    def mbr():
        return nbest_mbr(ids, nids, status, w, CN, max_len=max_len, ref=ref, ref_len=ref_len, want_dist=True)

    best, risk, flag, dist, _, _ = mbr()
    torch.cuda.synchronize()
    assert not flag.any().item()
    res["mdd_nbest_mbr"] = timed(mbr, reps, warmup)
    res["mdd_nbest_mbr_no_dist"] = timed(lambda: nbest_mbr(ids, nids, status, w, CN, max_len=max_len), reps, warmup)

    # the host entry over a sample of the same pairs; its distances must be the kernel's
    rs = np.random.default_rng(1)
    k = min(host_pairs, B * N * N)
    flat = rs.choice(B * N * N, size=k, replace=False) if k < B * N * N else np.arange(k)
    pairs = np.stack([flat // (N * N), (flat // N) % N, flat % N], axis=1)
    sec = host_align(ids_h, nids_h, pairs)
    res["host_pairs_timed"] = int(k)
    res["host_align_ms_scaled"] = sec * 1e3 * (B * N * N) / k
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import align_ids_batch
    bb, nn, mm = pairs[:2000].T
    ok = (nids_h[nn, bb] > 0) & (nids_h[mm, bb] > 0)
    d_host = align_ids_batch(ids_h[nn, bb], nids_h[nn, bb], ids_h[mm, bb], nids_h[mm, bb])[0]
    assert (d_host[ok] == dist.cpu().numpy()[bb, nn, mm][ok]).all(), "the kernel's distances differ from mdd_align_batch's"

    # rescoring and the search, on peaky posteriors
    T = 250 if max_len <= 64 else 600
    i2c = synth.phone_table_41()
    dec = BeamDecoder(i2c, beam_width=N, blank_index=0, space_idx=-1, lm_path=os.path.join(ROOT, "tests", "golden", "lm_synth45.arpa"), lm_alpha=0.0)
    lp = torch.from_numpy(np.stack([synth.peaky_logp(T, CN, 40, seed=9000 + b) for b in range(B)], axis=1)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ids_t = torch.zeros((N, B, T), dtype=torch.int32, device="cuda")
    ids_t[:, :, :max_len] = ids.clamp(min=1)                     # the list as labels: no blank
    res["T"] = T
    res["rescore"] = timed(lambda: dec.nbest_loglik(lp, lens, ids_t, nids, max_len=max_len), max(reps // 4, 5), 2, True)
    res["search_entry"] = "mdd_beam_nbest" if _lib.lib().mdd_beam_fits(T, B, CN, N) else "mdd_beam_wide"
    res["search"] = timed(lambda: dec.decode_nbest_ids(lp, lens, N), max(reps // 4, 5), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_pairs", type=int, default=20000)
    ap.add_argument("--shapes", type=int, nargs="+", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: the median needs at least 20 calls")
    res = dict(C=CN, reps=a.reps, warmup=a.warmup, shapes=[run(*SHAPES[i], a.reps, a.warmup, a.host_pairs) for i in a.shapes])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("Minimum-Bayes-risk decode of an N-best list (tools/time_mbr.py): C = %d, lists of a base sequence with 0-3 edits per hypothesis;\n"
                    "ms per call between HIP events, median [min .. max] of %d warm calls back to back (rescore, search: %d calls)\n"
                    % (CN, a.reps, max(a.reps // 4, 5)))
            for s in res["shapes"]:
                f.write("B = %d, N = %d, max_len = %d: %d pairs, mean length %.1f ids\n" % (s["B"], s["N"], s["max_len"], s["pairs"], s["mean_len"]))
                for k in ("mdd_nbest_mbr", "mdd_nbest_mbr_no_dist", "rescore", "search"):
                    v = s[k]
                    label = k if k != "search" else "search (%s, T = %d)" % (s["search_entry"], s["T"])
                    f.write("  %-36s %10.4f  [%.4f .. %.4f]\n" % (label, v["median_ms"], v["min_ms"], v["max_ms"]))
                f.write("  %-36s %10.1f  (one thread; %d of the pairs timed in one call and scaled to all)\n"
                        % ("host mdd_align_batch", s["host_align_ms_scaled"], s["host_pairs_timed"]))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
