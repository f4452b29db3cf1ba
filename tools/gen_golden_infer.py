#!/usr/bin/env python3
"""G13 golden generator -- TEST INFRASTRUCTURE, CPU only, runs only where the reference tree is present.

Runs the reference's OWN batch loop ``infer()`` (AA/infer.py:282-372, its function definition extracted with ast as
oracle/gen_golden.py's load_infer_functions does -- the module has import-time argparse and absent dependencies) over the
18 words of tests/golden/vocabulary_single that the CMU dictionary holds:

  features  oracle.stack_skip(apply_cmvn(fbank(wav)))  (Kaldi itself is absent: feature parity unpinned, as in G12)
  batches   the reference's create_input (AA/utils/data_loader.py:151-181, extracted with ast: its module imports the absent
            kaldiio), utterances in sorted order of their id as a string
  model     the reference's CTC_Model with synth_state_dict(REFERENCE, seed=11)
  decoder   the reference's BeamDecoder(beam 10, lm_synth45.arpa, alpha 0)

with the substitutions the package's infer mirror documents: args.wav_transcript_path is a temporary folder (its
decode_seq.txt is read back), phonetic.api_word_translation returns '', word_dict[utt]['ipa'] is the CMU pronunciation.
Two cases: batch_size=64 (one batch of 18, the recipe's setting) and batch_size=8 (three batches, each padded to its own
maximum).  Recorded per case: the captured stdout, the decode_seq.txt lines, the returned totals, and per batch its
utterances, input_sizes, T_max, L_max and log-probs.

Usage:  python tools/gen_golden_infer.py      (writes tests/golden/g13_infer.{json,npz})
"""
import ast
import contextlib
import io
import json
import math
import os
import string
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (puts the reference on sys.path; exits when it is absent)
from oracle import oracle as orc  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

AA, OUT, synth = gg.AA, gg.OUT, gg.synth
CASES = (64, 8)


def extract(path, names, ns):
    """exec the top-level function definitions `names` of a reference file in namespace `ns` (no module-level code)."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names), names
    exec(compile(ast.Module(body=body, type_ignores=[]), os.path.basename(path) + "<extract>", "exec"), ns)
    return ns


def lexicon():
    """The reference's CMU lookup (AA/dict/phonetic_dict.py load_cmudict / cmu_dict), as G12 extracts it."""
    src = open(os.path.join(AA, "dict", "phonetic_dict.py")).read()
    cls = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Phonetic"][0]
    meths = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("load_cmudict", "cmu_dict")]
    stub = ast.ClassDef(name="RefLexicon", bases=[], keywords=[], body=meths, decorator_list=[])
    ns = {"os": os, "__file__": os.path.join(AA, "dict", "phonetic_dict.py")}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), "phonetic_dict.py<lexicon>", "exec"), ns)
    lex = ns["RefLexicon"]()
    lex.cmudict_plain = {}
    return lex


def main():
    i2c = synth.phone_table_41()
    c2i = {v: k for k, v in i2c.items()}
    wdir = os.path.join(OUT, "vocabulary_single")
    stats = orc.read_cmvn_stats(os.path.join(OUT, "global_fbank_cmvn.txt"))
    lex = lexicon()
    utts = {}
    for i in range(1, 21):
        lines = open(os.path.join(wdir, "%d.txt" % i)).readlines()
        word = lines[-1].strip("\n")             # what wrd.txt hands back (AA/infer.py:531-532, 265-271)
        cmu = lex.cmu_dict(word)
        if not cmu:
            continue
        parts_ = [p.rstrip(string.digits) if p not in ["ER0", "AH0"] else p for p in cmu.split(" ")]   # infer.py:545-547
        canon = " ".join(p.lower() for p in parts_)
        wav, rate = orc_wav(os.path.join(wdir, "%d.wav" % i))
        assert rate == 16000
        feats = orc.stack_skip(orc.apply_cmvn(orc.fbank(wav), stats))
        utts[str(i)] = dict(word=word, cmu=cmu, canonical=canon, feats=feats, ids=[c2i[p] for p in canon.split()])
    order = sorted(utts)
    assert len(order) == 18, len(order)

    ns = {"torch": torch, "math": math}
    ns.update(gg.load_infer_functions())
    extract(os.path.join(AA, "infer.py"), ["infer"], ns)
    cins = extract(os.path.join(AA, "utils", "data_loader.py"), ["create_input"], {"torch": torch})["create_input"]
    geom = synth.Geometry(**synth.REFERENCE)
    model = gg.build_reference_model(geom, synth.synth_state_dict(geom, seed=11))
    beam = gg.BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(OUT, "lm_synth45.arpa"),
                          lm_alpha=0.0)
    vocab = types.SimpleNamespace(index2word=i2c, word2index=c2i)
    phonetic = types.SimpleNamespace(api_word_translation=lambda utterance: "")
    word_dict = {u: {"ipa": utts[u]["cmu"]} for u in order}
    transcripts = {u: utts[u]["word"] for u in order}

    meta = dict(order=order, utts={u: dict(word=utts[u]["word"], cmu=utts[u]["cmu"], canonical=utts[u]["canonical"],
                                           T=int(utts[u]["feats"].shape[0])) for u in order}, cases=[])
    arrays = {}
    for bs in CASES:
        batches = []
        for s in range(0, len(order), bs):
            chunk = order[s:s + bs]
            batches.append(cins([(torch.from_numpy(utts[u]["feats"]), torch.LongTensor(utts[u]["ids"]),
                                  torch.LongTensor(utts[u]["ids"]), u) for u in chunk]))
        captured = []

        def run_model(inputs, trans):
            with torch.no_grad():
                lp = model(inputs, trans)
            captured.append(lp.numpy().copy())
            return lp

        with tempfile.TemporaryDirectory() as tmp:
            ns["args"] = types.SimpleNamespace(wav_transcript_path=tmp)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                totals = ns["infer"](phonetic, word_dict, batches, torch.device("cpu"), run_model, beam, vocab, transcripts, False)
            seq = open(os.path.join(tmp, "decode_seq.txt")).read().splitlines()
        case = dict(batch_size=bs, stdout=buf.getvalue(), decode_seq=seq, totals=list(totals), batches=[])
        for k, (b, lp) in enumerate(zip(batches, captured)):
            inputs, sizes, _, _, trans, _, ulist = b
            arrays["bs%d_b%d_logp" % (bs, k)] = lp.astype(np.float32)
            arrays["bs%d_b%d_input_sizes" % (bs, k)] = sizes.numpy().astype(np.float32)
            case["batches"].append(dict(utts=list(ulist), T_max=int(inputs.shape[1]), L_max=int(trans.shape[1])))
        meta["cases"].append(case)
        print("G13 batch_size=%d: %d batches, totals %s" % (bs, len(batches), totals))
    np.savez_compressed(os.path.join(OUT, "g13_infer.npz"), **arrays)
    with open(os.path.join(OUT, "g13_infer.json"), "w") as f:
        json.dump(meta, f, indent=1)


def orc_wav(path):
    import wave
    w = wave.open(path)
    assert w.getnchannels() == 1 and w.getsampwidth() == 2
    return np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).astype(np.float32), w.getframerate()


if __name__ == "__main__":
    main()
