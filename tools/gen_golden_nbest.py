#!/usr/bin/env python3
"""G16 golden generator -- TEST INFRASTRUCTURE, CPU only, runs only where the reference tree is present; no test runs it.

Runs the reference's OWN beam search (AA/utils/BeamSearch.py through AA/utils/ctcDecoder.BeamDecoder, tests/golden/lm_synth45.arpa) and
records what its ending computes before it keeps the head: ``BeamState.sort`` is wrapped to note ``(y, prTotal)`` of every entry in
the order it returns them, and the note of the last call of an utterance -- the sort of the EOS-scored, length-normalised final state
(BeamSearch.py:148) -- is the ranked N-best list.

Utterances (C = 45, T <= 40, one decode call each):
  peaky / flat   beams 3, 10 and 20 x lm_alpha 0 and 0.25
  tied           class groups with bit-identical posteriors, alpha 0: exact ties inside the list (asserted here)
  errors         all-blank (IndexError), a zero posterior (ValueError), a unigram the LM lacks (KeyError; lm_synth45_missing.arpa)

Written: tests/golden/g16_nbest.npz (the log-posteriors and the two dense LM tables) and g16_nbest.json (per utterance: length, beam,
alpha, LM, the error name or the ranked id lists with their scores; floats round-trip exactly through repr).

Usage:  python tools/gen_golden_nbest.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (the paths and synth; imports the reference; exits when its tree is absent)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import utils.BeamSearch as uBeam  # noqa: E402  (reference)

OUT, synth, C = gg.OUT, gg.synth, 45
_LAST = []


def _recording_sort(self, _orig=uBeam.BeamState.sort):
    ys = _orig(self)
    _LAST[:] = [(y, self.entries[y].prTotal) for y in ys]
    return ys


uBeam.BeamState.sort = _recording_sort


def tied_logp(T, seed):
    """Classes fall into 11 groups whose members share their logits: group mates are bit-identical on every frame."""
    rs = np.random.Generator(np.random.PCG64(seed))
    group = rs.permutation(C) % 11
    z = rs.standard_normal((T, 11))[:, group]
    z[:, 0] -= 0.5
    lp = gg.logsoftmax32(z)
    for g in range(11):
        members = np.nonzero((group == g) & (np.arange(C) != 0))[0]
        assert (lp[:, members] == lp[:, members[:1]]).all()
    return lp


def utterances():
    rs = np.random.Generator(np.random.PCG64(1600))
    out = []
    for beam in (3, 10, 20):
        for alpha in (0.0, 0.25):
            out.append(("peaky", synth.peaky_logp(40, C, 12, seed=1600 + beam), 40, beam, alpha, "lm45"))
            T = 20
            out.append(("flat", gg.logsoftmax32(rs.standard_normal((T, C))), T - (beam % 4), beam, alpha, "lm45"))
    for i, beam in enumerate((3, 10, 20)):
        out.append(("tied", tied_logp(12, 1650 + i), 12, beam, 0.0, "lm45"))
    T = 12
    allblank = gg.logsoftmax32(np.concatenate([np.full((T, 1), 14.0), np.zeros((T, C - 1))], axis=1))
    z = np.random.Generator(np.random.PCG64(3)).standard_normal((T, C))
    z[:, 2] = -300.0
    out.append(("allblank", allblank, T, 10, 0.0, "lm45"))
    out.append(("underflow", gg.logsoftmax32(z), T, 10, 0.25, "lm45"))
    out.append(("missing_unigram", synth.peaky_logp(T, C, 4, seed=8), T, 10, 0.25, "lm45_missing"))
    return out


def main():
    i2c = synth.phone_table_41()
    arpa = {"lm45": os.path.join(OUT, "lm_synth45.arpa"), "lm45_missing": os.path.join(OUT, "lm_synth45_missing.arpa")}
    arrays = {name: gg.lm_table(gg.LanguageModel(arpa_file=path), i2c, C) for name, path in arpa.items()}
    recs, tied_lists, errors = [], 0, set()
    for u, (kind, lp, ln, beam, alpha, lm) in enumerate(utterances()):
        dec = gg.BeamDecoder(i2c, beam_width=beam, blank_index=0, space_idx=-1, lm_path=arpa[lm], lm_alpha=alpha)
        _LAST[:] = []
        rec = dict(kind=kind, len=ln, beam=beam, alpha=alpha, lm=lm, error=None, ids=[], scores=[], best=None)
        try:
            rec["best"] = dec.decode(torch.from_numpy(lp).unsqueeze(1), [ln])[0]
            assert len(_LAST) == beam and rec["best"] == " ".join(i2c[k] for k in _LAST[0][0])
            rec["ids"] = [[int(k) for k in y] for y, _ in _LAST]
            rec["scores"] = [float(s) for _, s in _LAST]
            tied_lists += any(a == b for a, b in zip(rec["scores"], rec["scores"][1:]))
        except (IndexError, ValueError, KeyError) as e:
            rec["error"] = type(e).__name__
            errors.add(rec["error"])
        arrays["u%d" % u] = lp
        recs.append(rec)
        print("G16 %2d %-16s beam %2d alpha %.2f -> %s" % (u, kind, beam, alpha, rec["error"] or rec["best"]))
    assert tied_lists >= 2 and errors == {"IndexError", "ValueError", "KeyError"}, (tied_lists, errors)
    np.savez_compressed(os.path.join(OUT, "g16_nbest.npz"), **arrays)
    with open(os.path.join(OUT, "g16_nbest.json"), "w") as f:
        json.dump(dict(C=C, blank=0, utterances=recs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
