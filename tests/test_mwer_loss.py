"""train.MWERLoss on the GPU, on the lists the GPU beam search actually returns (synth.peaky_logp posteriors with softened peaks, so that
the list's posterior is spread over several hypotheses; the synthetic bigram table of tests/golden/).

  1. the loss is mwer_weight * sum ref_risk + ctc_weight * sum nll, both from the separate entries;
  2. the gradient against the float64 yardstick (tests/ctc_nbest_grad_cases.risk_f64) on the same list, per utterance within
         GRAD_ATOL sum_n |coef_n|  +  2 LOGLIK_RTOL max_n |loglik_n| sum_n P_n |cost_n - R|
     -- the lattice bound, and what the project's own 1e-6 relative bound on a log-likelihood can move the coefficients (|g_n| <= 1);
  3. the per-rank route, forced, against the one-launch route within 2 GRAD_ATOL sum |coef| (each is a linear combination of tensors held to
     GRAD_ATOL, with the same coefficients); and with the one-launch log-likelihoods refused as well, where the coefficients come from
     log-likelihoods rounded through fp32 (6e-8 relative, inside LOGLIK_RTOL), within the sum of that and bound 2's second term;
  4. through the model (synth.TINY): every parameter gets a finite gradient, and with mwer_weight = 0 the gradients are ctc_weight times
     CTCLoss's (ctc_weight a power of two, so the scaling itself is exact);
  5. the program: steps.train_ctc.main with mwer_nbest and init_model on the small WAV corpus of tests/test_train_wav.py."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import ctc_nbest_grad_cases as gc
from tests.helpers import GOLD, record_margin

pytestmark = pytest.mark.gpu
ARPA = os.path.join(GOLD, "lm_synth45.arpa")
T, B, CN, N, BEAM = 40, 4, 12, 5, 8


def _decoder(beam=BEAM):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(synth.phone_table_41(), beam_width=beam, blank_index=0, space_idx=-1, lm_path=ARPA, lm_alpha=0.2)


@functools.lru_cache(maxsize=None)
def _inputs():
    """(lp [T,B,C], lens, targets [B,Lt], target lengths): soft peaks, so that several hypotheses share the list's posterior."""
    from ctc_attention_mispronunciation_amd import synth
    lp = np.stack([synth.peaky_logp(T, CN, 5 + b, seed=5100 + b, blank_boost=2.5, peak_boost=3.0) for b in range(B)], axis=1)
    lens = np.array([T, 36, 31, T], dtype=np.int64)
    # targets near the lists: the greedy reading of the utterance (argmax, repeats merged, blanks dropped) without its first phone, so that
    # the listed hypotheses, which differ from one another by an edit or two, lie at different distances from it
    tg, tl = np.zeros((B, T), dtype=np.int64), np.zeros((B,), dtype=np.int64)
    for b in range(B):
        best = lp[:lens[b], b].argmax(axis=-1)
        seq = [int(c) for t, c in enumerate(best) if c != 0 and (t == 0 or c != best[t - 1])][1:]
        tg[b, :len(seq)], tl[b] = seq, len(seq)
    tg = tg[:, :max(int(tl.max()), 1)].copy()
    assert (tl >= 2).all()
    for a in (lp, lens, tg, tl):
        a.setflags(write=False)
    return lp, lens, tg, tl


def _loss(per_rank=False, mwer_weight=1.0, ctc_weight=0.0, want_grad=True):
    from ctc_attention_mispronunciation_amd.train import MWERLoss
    lp, lens, tg, tl = _inputs()
    x = torch.from_numpy(np.array(lp)).cuda().requires_grad_(want_grad)
    fn = MWERLoss(_decoder(), N, ctc_weight=ctc_weight, mwer_weight=mwer_weight, per_rank=per_rank)
    loss = fn(x, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(lens)), torch.from_numpy(np.array(tl)))
    if want_grad:
        loss.backward()
    return fn, loss, None if x.grad is None else x.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fused():
    fn, loss, grad = _loss()
    assert fn.last["fused"] and not bool(fn.last["status"].any()) and not bool(fn.last["flag"].any())
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in fn.last.items()}, float(loss.detach()), grad


@functools.lru_cache(maxsize=None)
def _yardstick():
    last, _, _ = _fused()
    lp, lens, tg, tl = _inputs()
    width = max(int(last["nids"].max()), 1)
    r = gc.risk_f64(lp, lens, last["ids"], last["nids"], last["ref_dist"], max_len=width)
    spread = (r.post * np.abs(last["ref_dist"] - r.risk[None, :])).sum(axis=0)           # sum_n P_n |cost_n - R| = sum_n |coef_n|
    ll = np.where(np.isfinite(r.nll), r.nll, 0.0)
    return r, spread, np.abs(ll).max(axis=0)


def test_the_list_is_worth_testing_on():
    """The inputs' own condition: every utterance has at least two feasible hypotheses with different costs and a spread posterior."""
    r, spread, _ = _yardstick()
    print("sum_n |coef_n| per utterance:", spread, "posterior of rank 0:", r.post[0])
    assert (spread > 1e-2).all() and (np.isfinite(r.nll).sum(axis=0) >= 2).all()


def test_loss_is_the_separate_entries_sum():
    from ctc_attention_mispronunciation_amd import hip_model
    lp, lens, tg, tl = _inputs()
    fn, loss, _ = _loss(mwer_weight=0.7, ctc_weight=0.25, want_grad=False)
    dec = _decoder()
    x = torch.from_numpy(np.array(lp)).cuda()
    lens_d = torch.from_numpy(np.array(lens)).cuda().int()
    ids, nids, status, _ = dec.decode_nbest_ids(x, lens_d, N)
    within = torch.arange(ids.shape[2], device="cuda").view(1, 1, -1) < nids.unsqueeze(-1)      # (ids behind a row's length are not written)
    assert torch.equal(nids, fn.last["nids"]) and torch.equal(ids[within], fn.last["ids"][within])
    ll = hip_model.ctc_nbest(x, lens_d, ids, nids, max_len=int(nids.max())).cpu().numpy()
    e = np.zeros_like(ll)
    for b in range(B):
        fin = np.isfinite(ll[:, b])
        e[:, b] = np.where(fin, np.exp(np.where(fin, ll[:, b], 0.0) - ll[fin, b].max()), 0.0)
    post = e / e.sum(axis=0)
    ref_risk = hip_model.nbest_mbr(ids, nids, status, torch.from_numpy(post), CN, ref=torch.from_numpy(np.array(tg)).int(),
                                   ref_len=torch.from_numpy(np.array(tl)).int())[5].cpu().numpy()
    nll = hip_model.ctc_loss(x, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(lens)), torch.from_numpy(np.array(tl)), want_grad=False)[0]
    want = 0.7 * ref_risk.sum() + 0.25 * float(nll.double().sum())
    assert np.isfinite(want) and abs(float(loss.detach()) - want) <= 1e-6 * abs(want), (float(loss.detach()), want)     # the value is returned in fp32
    assert np.abs(fn.last["risk"].cpu().numpy() - ref_risk).max() <= 1e-12 * ref_risk.max()


def test_gradient_against_the_float64_risk():
    last, loss, grad = _fused()
    r, spread, llmax = _yardstick()
    assert np.abs(last["post"] - r.post).max() <= 1e-4 and abs(loss - r.risk.sum()) <= 1e-4 * r.risk.sum()
    worst = 0.0
    for b in range(B):
        bound = gc.GRAD_ATOL * np.abs(r.coef[:, b]).sum() + 2 * gc.LOGLIK_RTOL * llmax[b] * spread[b]
        err = float(np.abs(grad[:, b].astype(np.float64) - r.grad[:, b]).max())
        print("b %d: |grad - f64| %.3e, bound %.3e (lattice %.3e + coefficients %.3e)" % (b, err, bound, gc.GRAD_ATOL * np.abs(r.coef[:, b]).sum(),
                                                                                        2 * gc.LOGLIK_RTOL * llmax[b] * spread[b]))
        worst = max(worst, err / bound)
        assert (grad[int(_inputs()[1][b]):, b] == 0).all()
    record_margin("ctc_nbest_grad_mwer_over_bound", worst, 1.0)
    assert worst <= 1.0, worst
    assert np.abs(grad).max() > 1e-3


def test_per_rank_route_agrees_with_the_one_launch_route(monkeypatch):
    from ctc_attention_mispronunciation_amd import hip_model
    last, loss, grad = _fused()
    r, spread, llmax = _yardstick()
    fn, loss2, grad2 = _loss(per_rank=True)
    assert not fn.last["fused"] and loss2.item() == loss
    assert np.array_equal(fn.last["coef"].cpu().numpy(), last["coef"])
    sums = np.abs(last["coef"]).sum(axis=0)
    for b in range(B):
        err = float(np.abs(grad2[:, b] - grad[:, b]).max())
        print("forced per-rank b %d: %.3e (bound %.3e)" % (b, err, 2 * gc.GRAD_ATOL * sums[b]))
        assert err <= 2 * gc.GRAD_ATOL * sums[b], (b, err)
    # the shape refused altogether: log-likelihoods from mdd_ctc_loss too, rounded through fp32
    monkeypatch.setattr(hip_model, "ctc_nbest_fits", lambda *a: False)
    fn, loss3, grad3 = _loss()
    assert not fn.last["fused"] and abs(loss3.item() - loss) <= 1e-5 * abs(loss)
    for b in range(B):
        err = float(np.abs(grad3[:, b] - grad[:, b]).max())
        bound = 2 * gc.GRAD_ATOL * sums[b] + 2 * gc.LOGLIK_RTOL * llmax[b] * spread[b]
        print("refused shape b %d: %.3e (bound %.3e)" % (b, err, bound))
        assert err <= bound, (b, err, bound)


# ------------------------------------------------------------------------------------------------------------------ model
def _train_model(geom, sd):
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    if (geom.emb_rows, geom.emb_dim) != (44, 512):       # (tests/test_train_geometry.py: the class builds the reference's table)
        model.embeds = nn.Embedding(geom.emb_rows, geom.emb_dim)
        model.lstm_embeds = nn.LSTM(geom.emb_dim, geom.hidden, batch_first=True, bidirectional=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.cuda().train()


def test_through_the_model():
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.train import CTCLoss, MWERLoss
    geom = synth.Geometry(**synth.TINY)
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, 5300, 4, 32, 5, 3)

    def grads(loss_fn):
        model = _train_model(geom, sd)
        model._dropout_masks = [torch.from_numpy(m) for m in masks]
        out = model(torch.from_numpy(x).cuda(), torch.from_numpy(x1).cuda())
        loss = loss_fn(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / 4
        loss.backward()
        return float(loss.detach()), {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}

    dec = _decoder()
    loss, g = grads(MWERLoss(dec, 3, ctc_weight=0.01, mwer_weight=1.0))
    assert np.isfinite(loss) and len(g) > 10
    for k, v in g.items():
        assert np.isfinite(v).all(), k
    assert max(float(np.abs(v).max()) for v in g.values()) > 0
    loss_c, g_c = grads(CTCLoss(reduction="sum"))
    loss_0, g_0 = grads(MWERLoss(dec, 3, ctc_weight=0.5, mwer_weight=0.0))
    assert abs(loss_0 - 0.5 * loss_c) <= 1e-6 * abs(loss_c)
    for k in g_c:
        scale = max(float(np.abs(g_c[k]).max()), 1e-30)
        assert float(np.abs(g_0[k] - 0.5 * g_c[k]).max()) <= 1e-6 * scale, k


# ---------------------------------------------------------------------------------------------------------------- program
def test_train_program_with_mwer_and_init_model(tmp_path, capsys):
    from tests import test_train_wav as tw
    from ctc_attention_mispronunciation_amd.steps import train_ctc
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.utils.data_loader import TrainWavLoader, Vocab
    fb = tw._fb()
    _, _, can, lab, units = tw._corpus()
    (tmp_path / "units").write_text(units)
    rec = tw._recorded()
    for split, count in (("train", 8), ("dev", 4)):
        os.makedirs(str(tmp_path / split))
        scp, labs, trans = [], [], []
        for i in range(count):
            n = 6400 + 160 * i
            x = rec[300 * i:300 * i + n] + 0.3 * tw._signal(n, 60 + i) if i % 2 == 0 else tw._signal(n, 60 + i)
            tw._write_wav(tmp_path / split / ("%s%d.wav" % (split, i)), x)
            scp.append("%s%d %s\n" % (split, i, tmp_path / split / ("%s%d.wav" % (split, i))))
            labs.append("%s%d %s\n" % (split, i, " ".join(lab[i % len(lab)].split()[:3])))
            trans.append("%s%d %s\n" % (split, i, " ".join(can[i % len(can)].split()[:4])))
        (tmp_path / split / "wav.scp").write_text("".join(scp))
        (tmp_path / split / "phn_text").write_text("".join(labs))
        (tmp_path / split / "transcript_phn_text").write_text("".join(trans))
    conf = dict(exp_name="first", checkpoint_dir=str(tmp_path / "ckpt"), vocab_file=str(tmp_path / "units"),
                train_wav_scp=str(tmp_path / "train" / "wav.scp"), train_lab_path=str(tmp_path / "train" / "phn_text"),
                train_trans_path=str(tmp_path / "train" / "transcript_phn_text"),
                valid_wav_scp=str(tmp_path / "dev" / "wav.scp"), valid_lab_path=str(tmp_path / "dev" / "phn_text"),
                valid_trans_path=str(tmp_path / "dev" / "transcript_phn_text"), cmvn_path=str(tmp_path / "cmvn" / "global_fbank_cmvn.txt"),
                left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2, num_workers=0, shuffle_train=True, feature_dim=81,
                output_class_dim=41, mel=False, feature_type="fbank", rnn_input_size=243, rnn_hidden_size=20, rnn_layers=1,
                rnn_type="nn.LSTM", bidirectional=True, batch_norm=True, drop_out=0.2, add_cnn=True, layers=2, channel="[(1, 4), (4, 4)]",
                kernel_size="[(3, 3), (3, 3)]", stride="[(1, 2), (2, 2)]", padding="[(1, 1), (1, 1)]", pooling="None",
                activation_function="relu", use_gpu=True, init_lr=0.001, num_epoches=1, end_adjust_acc=2, lr_decay=0.5, batch_size=4,
                weight_decay=0.0005, seed=1234, verbose_step=1)
    first = train_ctc.main(conf)
    capsys.readouterr()
    conf2 = dict(conf, exp_name="mwer", mwer_nbest=3, init_model=first, lm_path=ARPA, lm_alpha=0.2)
    best = train_ctc.main(conf2)
    out = capsys.readouterr().out
    for line in ("Initial weights from %s" % first, "MWER training: 3-best of beam 10, mwer_weight 1, ctc_weight 0.01", "Start training epoch: 1, learning_rate: 0.00100",
                 "Epoch = 1, step = 2, total_loss = ", "Epoch 1 Train done, total_loss: ", "Epoch 1 Valid done, total_loss: ", "epoch 1 done, cv acc is: ",
                 "adjust_rate_count:0 adjust_time:0", "End training, best dev loss is: "):
        assert line in out, line
    assert best == os.path.join(conf["checkpoint_dir"], "mwer", "ctc_best_model.pkl") and os.path.isfile(best)
    printed = float(re.search(r"Epoch 1 Valid done, total_loss: ([0-9.eE+-]+|nan|inf),", out).group(1))
    # the validation loss is the CTC one: CTCLoss over the dev set on the weights the run left
    package = torch.load(best, map_location="cpu", weights_only=False)
    model = CTC_Model(rnn_param=package["rnn_param"], add_cnn=package["add_cnn"], cnn_param=package["cnn_param"], num_class=package["num_class"],
                      drop_out=package["_drop_out"])
    model.load_state_dict(package["state_dict"])
    model = model.cuda()
    items = train_ctc.wav_items(conf["valid_wav_scp"], conf["valid_lab_path"], conf["valid_trans_path"])
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(conf["cmvn_path"]))
    loader = TrainWavLoader(items, Vocab(conf["vocab_file"]), 4, train=False, shuffle=False, cmvn=cmvn, right_ctx=2, n_skip_frame=2, n_downsample=2)
    _, dev_loss = train_ctc.run_epoch(1, model, loader, CTCLoss(reduction="sum"), torch.device("cuda:0"), is_training=False)
    assert np.isfinite(printed) and abs(dev_loss - printed) <= 1e-4 * abs(printed) + 1e-4, (dev_loss, printed)      # (printed with four decimals)
    assert package["dev_loss_results"] and abs(package["dev_loss_results"][0] - dev_loss) <= 1e-6 * abs(dev_loss)
    # the weights moved from the first run's
    w0 = torch.load(first, map_location="cpu", weights_only=False)["state_dict"]
    assert any(not torch.equal(w0[k], package["state_dict"][k]) for k in w0 if w0[k].dtype == torch.float32)
