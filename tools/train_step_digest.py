"""Bit identity of the training step between two builds of libmdd_hip.so.  Per library a child process (MDD_LIB_PATH, as
tests/test_gpu_parity.py selects its twin build) runs every case for two full steps -- train-mode forward with the dropout masks of
synth.train_case handed in, the product CTCLoss(sum)/B, backward, the product Adam step -- and prints the tensor table of
mdd_train_tensor_info and one SHA-256 per (case, mode, step) over the log-probs, the loss, every gradient, every running statistic
and every parameter after Adam.

    python tools/train_step_digest.py                      the digests of the package's own library
    python tools/train_step_digest.py --parent OLD.so [--out NOTES.txt] [--table TABLE.json]
        OLD.so twice, then the package's library.  A record is comparable when OLD.so repeats itself on it (BatchNorm statistics are
        fp64 atomics, so a bf16x3 record might not); every f32 and f32x6 record must be comparable, every comparable record must be
        identical in the new library.  Exit status 1 otherwise.  --table writes OLD.so's tensor tables (tests/golden/train_tensor_table.json).

Cases: the five shapes of test_train_step_split_bf16_variant (2560 rows: every split-K rule with more than one chunk; B = 272: the
per-step backward beside the persistent forward; T' = 2 and L = 1) and the tiny geometry of g11_train.json entry 0 (classifier
contraction below 1024: unsplit), each in modes f32, bf16x3 and f32x6; the first shape once more in f32 with MDD_TRAIN_CONV1_IM2COL=1.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(384, 32, 160, 12), (256, 272, 16, 5), (256, 100, 24, 5), (384, 7, 40, 6), (256, 2, 4, 1)]      # (H, B, T, L)
MODES = ("f32", "bf16x3", "f32x6")


def cases():
    """(name, geometry, seed, B, T, L, Lt, mode, im2col)"""
    from ctc_attention_mispronunciation_amd import synth
    out = []
    for H, B, T, L in SHAPES:
        geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
        for mode in MODES:
            out.append(("H%d_B%d_T%d_L%d" % (H, B, T, L), geom, 77, B, T, L, max(1, min(6, T // 4)), mode, False))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "g11_train.json")))[0]
    for mode in MODES:
        out.append(("tiny", synth.Geometry(**meta["geom"]), meta["seed"], meta["B"], meta["T"], meta["L"], meta["Lt"], mode, False))
    H, B, T, L = SHAPES[0]
    out.append(("H%d_B%d_T%d_L%d_im2col" % (H, B, T, L), synth.Geometry(**dict(synth.REFERENCE, hidden=H)), 77, B, T, L, 6, "f32", True))
    return out


def child():
    import numpy as np
    import torch
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.steps.train_ctc import build_training
    tables = {}
    for name, geom, seed, B, T, L, Lt, mode, im2col in cases():
        sd, x, x1, masks, tg, il, tl = synth.train_case(geom, seed, B, T, L, Lt)
        model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
        if geom.emb_rows != 44 or geom.emb_dim != 512:          # tiny geometry (as oracle/gen_golden.py builds the reference)
            model.embeds = nn.Embedding(geom.emb_rows, geom.emb_dim)
            model.lstm_embeds = nn.LSTM(geom.emb_dim, geom.hidden, batch_first=True, bidirectional=True)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        model = model.cuda().train()
        model.train_precision = mode
        model._dropout_masks = [torch.from_numpy(m) for m in masks]
        loss_fn, opt = build_training(model)
        xd, x1d = torch.from_numpy(x).cuda(), torch.from_numpy(x1).cuda()
        if im2col:
            os.environ["MDD_TRAIN_CONV1_IM2COL"] = "1"          # read when the handle is created, by the first forward
        for step in (1, 2):
            out = model(xd, x1d)
            os.environ.pop("MDD_TRAIN_CONV1_IM2COL", None)
            loss = loss_fn(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / B
            opt.zero_grad()
            loss.backward()
            h = hashlib.sha256()
            h.update(out.detach().cpu().numpy().tobytes())
            h.update(loss.detach().cpu().numpy().tobytes())
            for _, p in model.named_parameters():
                h.update(p.grad.cpu().numpy().tobytes())
            opt.step()
            for k, b in model.named_buffers():
                if "running_" in k:
                    h.update(b.cpu().numpy().tobytes())
            for _, p in model.named_parameters():
                h.update(p.detach().cpu().numpy().tobytes())
            print("DIGEST %s %s %d %s" % (name, mode, step, h.hexdigest()), flush=True)
        th = model._train_handle
        tables["tiny" if name == "tiny" else "reference_H%d" % geom.hidden] = [[k, n, int(b)] for k, n, b in zip(th.keys, th.numel, th.is_buffer)]
    print("TABLES " + json.dumps(tables, sort_keys=True), flush=True)


def run(lib):
    env = dict(os.environ)
    env.pop("MDD_TRAIN_CONV1_IM2COL", None)
    env.pop("MDD_TRAIN_PRECISION", None)
    if lib:
        env["MDD_LIB_PATH"] = os.path.abspath(lib)
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    digests, tables = {}, None
    for line in proc.stdout:
        f = line.split()
        if line.startswith("DIGEST "):
            digests[(f[1], f[2], int(f[3]))] = f[4]
            print(".", end="", flush=True)                      # progress: one dot per record
        elif line.startswith("TABLES "):
            tables = json.loads(line[7:])
    print(flush=True)
    if proc.wait() != 0 or tables is None:
        sys.exit("the child on %s failed with status %d" % (lib or "the package's library", proc.returncode))
    return digests, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.parent:
        digests, tables = run(None)
        for k, v in tables.items():
            print("table %s: %s" % (k, " ".join("%s:%d:%d" % tuple(e) for e in v)))
        for (name, mode, step), d in digests.items():
            print("%-28s %-7s step %d  %s" % (name, mode, step, d))
        return 0
    (p1, t1), (p2, t2), (new, tn) = run(args.parent), run(args.parent), run(None)
    lines, bad, skipped, same = [], [], [], 0
    lines.append("%-28s %-7s %-4s %-16s %-16s %-16s %s" % ("case", "mode", "step", "parent run 1", "parent run 2", "new", "verdict"))
    for key in p1:
        name, mode, step = key
        if p1[key] != p2.get(key):
            verdict = "not comparable (the parent does not repeat itself)"
            skipped.append(key)
            if mode != "bf16x3":
                bad.append(key)
        elif new.get(key) == p1[key]:
            verdict, same = "identical", same + 1
        else:
            verdict = "DIFFERENT"
            bad.append(key)
        lines.append("%-28s %-7s %-4d %-16s %-16s %-16s %s" % (name, mode, step, p1[key][:16], (p2.get(key) or "-")[:16], (new.get(key) or "-")[:16], verdict))
    tables_same = t1 == tn
    lines.append("tensor tables (key, numel, is_buffer) of %s: %s" % (", ".join(sorted(t1)), "identical" if tables_same else "DIFFERENT"))
    ok = not bad and tables_same and set(new) == set(p1)
    lines.append("verdict: %s -- %d records, %d comparable and identical, %d not comparable%s" % (
        "PASS" if ok else "FAIL", len(p1), same, len(skipped), (" " + str(skipped)) if skipped else ""))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    if args.table:
        os.makedirs(os.path.dirname(os.path.abspath(args.table)), exist_ok=True)
        json.dump(t1, open(args.table, "w"), indent=0, sort_keys=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
