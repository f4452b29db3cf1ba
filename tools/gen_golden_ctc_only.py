#!/usr/bin/env python3
"""G15 golden generator -- TEST INFRASTRUCTURE, CPU only, runs only where the reference tree is present.

Runs the reference's OWN CTC-only baseline model, ``CTC_Model`` of egs/cnn-rnn-ctc ("CRC") models/cnn_rnn.py, in eval mode and
float32 on ``synth_state_dict(Geometry(ctc_only=True, ...), seed)`` for three geometries:

  tiny   feat 15, H 8, 2 layers, C 7, 4 channels
  h256   feat 243, H 256, 4 layers, C 45
  h384   feat 243, H 384, 4 layers, C 45   (CRC/conf/ctc_config.yaml)

on a batch of B = 3, T = 32 with ragged lengths (synth_batch).  Recorded per geometry: the inputs, the length fractions, the
reference's log-probs and the ordered list of its float ``state_dict`` keys with their shapes.  For h384 also what the reference's
decoders (CRC/utils/ctcDecoder.py: GreedyDecoder, BeamDecoder beam 10 with tests/golden/lm_synth45.arpa, alpha 0) give on those
log-probs.

Usage:  python tools/gen_golden_ctc_only.py      (writes tests/golden/g15_ctc_only.{json,npz})
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (the paths and synth; exits when the reference tree is absent)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

OUT, synth = gg.OUT, gg.synth
CRC = os.path.join(os.path.dirname(gg.AA), "cnn-rnn-ctc")

# oracle.gen_golden has the attention recipe's `models` and `utils` packages imported; the baseline recipe uses the same names
for name in [n for n in sys.modules if n.split(".")[0] in ("models", "utils")]:
    del sys.modules[name]
sys.path.remove(gg.AA)
sys.path.insert(0, CRC)
from models.cnn_rnn import CTC_Model  # noqa: E402  (reference, CTC-only)
from utils.ctcDecoder import GreedyDecoder, BeamDecoder  # noqa: E402  (reference, CTC-only recipe)

CASES = (("tiny", dict(feat=15, hidden=8, layers=2, num_class=7, channels=4), 21),
         ("h256", dict(synth.REFERENCE_256), 22),
         ("h384", dict(synth.REFERENCE), 23))
B, T, L = 3, 32, 6


def main():
    torch.set_num_threads(8)
    meta, arrays = dict(B=B, T=T, L=L, cases=[]), {}
    for tag, g, seed in CASES:
        geom = synth.Geometry(ctc_only=True, **g)
        sd = synth.synth_state_dict(geom, seed=seed)
        x, x1, frac, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=seed)
        model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})    # strict: the synthetic keys are the reference's
        model.eval()
        with torch.no_grad():
            logp = model(torch.from_numpy(x), torch.from_numpy(x1))
        assert logp.dtype == torch.float32 and tuple(logp.shape) == (T // 2, B, geom.num_class)
        keys = [[k, list(v.shape)] for k, v in model.state_dict().items() if v.is_floating_point()]
        assert len(keys) == 12 + 4 * geom.layers + 4 * (geom.layers - 1) + 5
        case = dict(tag=tag, geom=g, seed=seed, batch_seed=seed, keys=keys)
        arrays[tag + "_x"], arrays[tag + "_frac"], arrays[tag + "_logp"] = x, frac, logp.numpy()
        if tag == "h384":
            i2c = synth.phone_table_41()
            lens = [int(v) for v in (torch.from_numpy(frac) * logp.shape[0]).long()]
            case["lens"] = lens
            case["greedy"] = GreedyDecoder(i2c, space_idx=-1, blank_index=0).decode(logp, lens)
            beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(OUT, "lm_synth45.arpa"), lm_alpha=0.0)
            case["beam10"] = beam.decode(logp, lens)
        meta["cases"].append(case)
        print("G15", tag, tuple(logp.shape), "%d keys" % len(keys))
    np.savez_compressed(os.path.join(OUT, "g15_ctc_only.npz"), **arrays)
    with open(os.path.join(OUT, "g15_ctc_only.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
