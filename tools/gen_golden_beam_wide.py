#!/usr/bin/env python3
"""G17 golden generator -- TEST INFRASTRUCTURE, CPU only, runs only where the reference tree is present; no test runs it.

Runs the reference's OWN beam search (AA/utils/BeamSearch.py through AA/utils/ctcDecoder.BeamDecoder, tests/golden/lm_synth45.arpa) at the
widths only mdd_beam_wide takes, and records the winner's string and the ranked final list as tools/gen_golden_nbest.py does
(``BeamState.sort`` wrapped; the last call of an utterance is the sort of the EOS-scored, length-normalised final state).

Two settings:
  default    ``BeamDecoder(int2char, lm_path=...)``: every other constructor argument at the reference's default (beam_width 200, lm_alpha 0.01)
  b100       beam_width 100, lm_alpha 0.25
Two batches of posteriors (C = 45, T = 40, B = 4, lengths 40 / 33 / 17 / 26): peaky and flat.  Each utterance is one decode call.

A batch must rank robustly: the GPU rounds exp() differently from torch.exp on about 1 % of the inputs, so the project's N-best yardstick
(tests/nbest_reference.py) must give the reference's ranked ids under both of its exp flavours, and neighbouring scores must be equal or
more than 2e-7 relative apart.  The seed of a batch is the first one from its start value that does; it is recorded.

Written: tests/golden/g17_beam_wide.npz (the two batches, the lengths, the dense LM table, and per setting / batch / utterance the ranked
ids as int8 rows padded with -1 and their float64 scores) and g17_beam_wide.json (the settings, seeds and winner strings).

Usage:  python tools/gen_golden_beam_wide.py
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (the paths and synth; imports the reference; exits when its tree is absent)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import utils.BeamSearch as uBeam  # noqa: E402  (reference)
from tests import nbest_reference as nr  # noqa: E402

OUT, synth, C, T, LENS = gg.OUT, gg.synth, 45, 40, (40, 33, 17, 26)
SETTINGS = {"default": {}, "b100": dict(beam_width=100, lm_alpha=0.25)}
GAP = 2e-7
_LAST = []


def _recording_sort(self, _orig=uBeam.BeamState.sort):
    ys = _orig(self)
    _LAST[:] = [(y, self.entries[y].prTotal) for y in ys]
    return ys


uBeam.BeamState.sort = _recording_sort


def batch(kind, seed):
    if kind == "peaky":
        return np.stack([synth.peaky_logp(T, C, 12, seed=seed * 10 + b) for b in range(len(LENS))], axis=1)
    rs = np.random.Generator(np.random.PCG64(seed))
    return np.stack([gg.logsoftmax32(rs.standard_normal((T, C))) for _ in LENS], axis=1)


def reference_lists(logp, i2c, arpa, kw):
    dec = gg.BeamDecoder(i2c, lm_path=arpa, **kw)
    out = []
    for b, ln in enumerate(LENS):
        _LAST[:] = []
        best = dec.decode(torch.from_numpy(logp[:, b:b + 1].copy()), [ln])[0]
        assert len(_LAST) == dec.beam_width and best == " ".join(i2c[k] for k in _LAST[0][0])
        out.append((best, [[int(k) for k in y] for y, _ in _LAST], [float(s) for _, s in _LAST]))
    default_alpha = inspect.signature(gg.BeamDecoder.__init__).parameters["lm_alpha"].default      # (the decoder object does not keep the value)
    return out, dec.beam_width, kw.get("lm_alpha", default_alpha)


def robust(logp, table, lists, beam, alpha):
    for flavour in nr.EXP_FLAVOURS:
        for (final, status), (_, ids, scores) in zip(nr.nbest(logp, LENS, table, beam, alpha, 0, flavour), lists):
            if status != 0 or [y for y, _ in final] != ids:
                return False
    for _, _, scores in lists:
        for s0, s1 in zip(scores, scores[1:]):
            if s0 != s1 and (s0 - s1) <= GAP * max(abs(s0), abs(s1)):
                return False
    return True


def main():
    i2c = synth.phone_table_41()
    arpa = os.path.join(OUT, "lm_synth45.arpa")
    table = gg.lm_table(gg.LanguageModel(arpa_file=arpa), i2c, C)
    arrays = {"lm45": table, "lens": np.asarray(LENS, dtype=np.int32)}
    meta = dict(C=C, T=T, blank=0, lens=list(LENS), settings={}, batches={})
    for kind, start in (("peaky", 1700), ("flat", 1750)):
        for seed in range(start, start + 50):
            logp = batch(kind, seed)
            got = {}
            for name, kw in SETTINGS.items():
                lists, beam, alpha = reference_lists(logp, i2c, arpa, kw)
                meta["settings"][name] = dict(beam=beam, alpha=alpha)
                if not robust(logp, table, lists, beam, alpha):
                    break
                got[name] = lists
            if len(got) == len(SETTINGS):
                break
            print("G17 %s seed %d: not robust, next" % (kind, seed))
        else:
            sys.exit("no robust seed for " + kind)
        arrays[kind] = logp
        meta["batches"][kind] = dict(seed=seed, best={name: [best for best, _, _ in lists] for name, lists in got.items()})
        for name, lists in got.items():
            for b, (best, ids, scores) in enumerate(lists):
                rows = np.full((len(ids), max(len(y) for y in ids)), -1, dtype=np.int8)
                for n, y in enumerate(ids):
                    rows[n, :len(y)] = y
                arrays["%s_%s_u%d_ids" % (name, kind, b)] = rows
                arrays["%s_%s_u%d_scores" % (name, kind, b)] = np.asarray(scores, dtype=np.float64)
                print("G17 %-7s %-5s u%d -> %s" % (name, kind, b, best))
    np.savez_compressed(os.path.join(OUT, "g17_beam_wide.npz"), **arrays)
    with open(os.path.join(OUT, "g17_beam_wide.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
