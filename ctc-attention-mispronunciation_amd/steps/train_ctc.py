"""The training loop around the hot path -- mirror of the reference's ``steps/train_ctc.py`` (AA/steps/train_ctc.py):

* ``run_epoch`` (:28-105)  one pass over a data loader: train-mode forward, ``loss_fn(out, targets, (frac * T').long(), target_sizes)
  / batch_size``, greedy frame error count through ``model.compute_wer``, ``zero_grad / backward / step``;  same arguments and
  ``(1 - error rate, mean loss)`` return.  With ``torch.distributed`` initialised, gradients are averaged over the ranks before the
  optimizer step (data-parallel config 5 of BASELINE.json: every rank steps its own 32-utterance shard; BatchNorm statistics stay
  per rank, the reference has no SyncBN).
* ``LrSchedule`` (:207-268)  the dev-loss driven halving the reference writes inline in ``main()``: a new best (by more than
  ``end_adjust_acc``) resets the patience; ten epochs inside the band, or one outside it, restore the best state, multiply the rate
  by ``decay`` and count an adjustment; eight adjustments stop training.
* ``build_training(...)``  model + ``CTCLoss(reduction='sum')`` + ``Adam(lr, weight_decay)`` as :184-187 wires them.
* ``main(conf)`` (:111-291) and ``python -m ctc_attention_mispronunciation_amd.steps.train_ctc --conf CONF``: the program -- seeds, data (the
  reference's ark route, or WAVs through ``TrainWavLoader`` with the CMVN statistics computed on the GPU if the file is absent), model from
  the conf, epoch loop, ``ctc_best_model.pkl``.
The arithmetic of every step runs in libmdd_hip (train.py); this file is host control flow only.
"""
import copy
import os
import sys

import torch

from ..train import Adam, CTCLoss


def allreduce_gradients(model, bucket_bytes=64 << 20):
    """Average the gradients over the ranks (RCCL all-reduce over xGMI on ROCm; no-op without an initialised process group).
    Gradients are packed into buckets of ~64 MB so the ring moves few large messages (21 M parameters = 85 MB: two buckets)."""
    import torch.distributed as dist
    import os
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not os.environ.get("MDD_FORCE_DIST")):
        return                                       # (MDD_FORCE_DIST: rehearse the collective path on a one-rank group)
    world = dist.get_world_size()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    bucket, size = [], 0

    def flush():
        if not bucket:
            return
        flat = torch.cat([g.reshape(-1) for g in bucket])
        if dist.get_backend() == "gloo" and flat.is_cuda:
            h = flat.cpu()
            dist.all_reduce(h)
            flat.copy_(h)
        else:
            dist.all_reduce(flat)
        flat.div_(world)
        off = 0
        for g in bucket:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()
    for g in grads:
        bucket.append(g)
        size += g.numel() * 4
        if size >= bucket_bytes:
            flush()
            bucket, size = [], 0
    flush()


def run_epoch(epoch_id, model, data_iter, loss_fn, device, optimizer=None, print_every=20, is_training=True):
    """AA/steps/train_ctc.py:28-105, same arguments, prints and return value.  The reference pulls the loss (``loss.item()``) and the
    frame argmax (``torch.max`` + ``compute_wer`` on numpy copies) to the host on EVERY step; at 14-33 ms per HIP step those two
    synchronisations are no longer free, so the bookkeeping stays on the device: the loss is accumulated in a float64 device
    scalar (the same sum, in the same order, as the reference's Python float), the greedy prediction of ``compute_wer``
    (argmax, drop repeats, drop blanks: model_ctc.py:227-244) is mdd_greedy's output, and both come to the host once per print
    interval, where the edit distances of all pending utterances are one native call (mdd_align_batch)."""
    import numpy as np
    from ..utils.ctcDecoder import GreedyDecoder, align_ids_batch
    model.train() if is_training else model.eval()
    total_loss, total_tokens, total_errs, i = 0, 0, 0, -1
    greedy = GreedyDecoder({}, space_idx=-1, blank_index=0)
    loss_acc, pending = None, []

    def flush():
        nonlocal total_loss, total_tokens, total_errs, loss_acc, pending
        if loss_acc is not None:
            total_loss = float(loss_acc.item())               # the one host synchronisation of the interval
        for ids, n, tg, tl in pending:
            ids, n, tg, tl = ids.cpu().numpy(), n.cpu().numpy(), tg.cpu().numpy().astype(np.int32), tl.cpu().numpy().astype(np.int32)
            dist = align_ids_batch(tg, tl, ids, n)[0]
            empty = dist < 0                                  # ed.eval with an empty side = the length of the other one
            total_errs += int(dist[~empty].sum()) + int(np.maximum(tl, n)[empty].sum())
            total_tokens += int(tl.sum())
        pending = []
    for i, data in enumerate(data_iter):
        inputs, input_sizes, targets, target_sizes, trans, trans_sizes, utt_list = data
        inputs, input_sizes = inputs.to(device), input_sizes.to(device)
        targets, target_sizes, trans = targets.to(device), target_sizes.to(device), trans.to(device)
        with torch.set_grad_enabled(is_training):
            out = model(inputs, trans)
            out_len, batch_size, _ = out.size()
            input_sizes = (input_sizes * out_len).long()
            loss = loss_fn(out, targets, input_sizes, target_sizes)
            loss = loss / batch_size
        if out.is_cuda:
            loss_acc = loss.detach().double() if loss_acc is None else loss_acc + loss.detach().double()
            ids, n = greedy.decode_ids(out.detach(), input_sizes)
            pending.append((ids, n, targets, target_sizes))
        else:                                                 # (CPU inputs: the forward has copied the posteriors back already)
            total_loss += loss.item()
            _, index = torch.max(out.detach(), dim=-1)
            batch_errs, batch_tokens = model.compute_wer(index.transpose(0, 1).cpu().numpy(), input_sizes.cpu().numpy(), targets.cpu().numpy(),
                                                         target_sizes.cpu().numpy())
            total_errs += batch_errs
            total_tokens += batch_tokens
        if (i + 1) % print_every == 0 and is_training:
            flush()
            print('Epoch = %d, step = %d, total_loss = %.4f, total_wer = %.4f' % (epoch_id, i + 1, total_loss / (i + 1), total_errs / total_tokens))
        if is_training:
            optimizer.zero_grad()
            loss.backward()
            allreduce_gradients(model)
            optimizer.step()
    flush()
    average_loss = total_loss / (i + 1)
    print("Epoch %d %s done, total_loss: %.4f, total_wer: %.4f" % (epoch_id, "Train" if is_training else "Valid", average_loss, total_errs / total_tokens))
    return 1 - total_errs / total_tokens, average_loss


class LrSchedule(object):
    """State machine of train_ctc.py:207-268.  Call ``begin_epoch()`` before an epoch (applies a pending decay to the optimizer,
    returns False when training must stop) and ``end_epoch(acc, dev_loss)`` after its validation pass."""

    def __init__(self, model, optimizer, init_lr, decay, end_adjust_acc, num_epoches):
        self.model, self.optimizer = model, optimizer
        self.learning_rate, self.decay, self.band, self.num_epoches = init_lr, decay, end_adjust_acc, num_epoches
        self.count = 0
        self.loss_best = self.loss_best_true = 1000
        self.adjust_rate_flag = self.stop_train = False
        self.adjust_time = 0
        self.adjust_rate_count = 0
        self.acc_best = 0
        self.model_state = self.op_state = self.best_model_state = self.best_op_state = None
        self.printed_count = self.printed_time = 0     # what train_ctc.py:256 prints: the counters before an adjustment resets them

    def begin_epoch(self):
        if self.stop_train or self.count >= self.num_epoches:
            return False
        self.count += 1
        if self.adjust_rate_flag:
            self.learning_rate *= self.decay
            self.adjust_rate_flag = False
            for group in self.optimizer.param_groups:
                group['lr'] *= self.decay
        return True

    def _snapshot(self):
        return copy.deepcopy(self.model.state_dict()), copy.deepcopy(self.optimizer.state_dict())

    def end_epoch(self, acc, dev_loss):
        if dev_loss < (self.loss_best - self.band):
            self.loss_best = self.loss_best_true = dev_loss
            self.adjust_rate_count = 0
            self.model_state, self.op_state = self._snapshot()
        elif dev_loss < self.loss_best + self.band:
            self.adjust_rate_count += 1
            if dev_loss < self.loss_best and dev_loss < self.loss_best_true:
                self.loss_best_true = dev_loss
                self.model_state, self.op_state = self._snapshot()
        else:
            self.adjust_rate_count = 10
        if acc > self.acc_best:
            self.acc_best = acc
            self.best_model_state, self.best_op_state = self._snapshot()
        self.printed_count, self.printed_time = self.adjust_rate_count, self.adjust_time
        if self.adjust_rate_count == 10:
            self.adjust_rate_flag = True
            self.adjust_time += 1
            self.adjust_rate_count = 0
            if self.loss_best > self.loss_best_true:
                self.loss_best = self.loss_best_true
            self.model.load_state_dict(self.model_state)
            self.optimizer.load_state_dict(self.op_state)
        if self.adjust_time == 8:
            self.stop_train = True

    def finish(self):
        """Load the best-accuracy state (train_ctc.py:283-285) before the checkpoint is written."""
        if self.best_model_state is not None:
            self.model.load_state_dict(self.best_model_state)
            self.optimizer.load_state_dict(self.best_op_state)


def build_training(model, init_lr=1e-3, weight_decay=5e-4):
    """(loss_fn, optimizer) as train_ctc.py:186-187 creates them."""
    return CTCLoss(reduction='sum'), Adam(model.parameters(), lr=init_lr, weight_decay=weight_decay)


# ---------------------------------------------------------------------------------------------------------------- the program
SUPPORTED_RNN = ("nn.LSTM", "nn.GRU", "nn.RNN")
SUPPORTED_ACTIVATE = ("relu", "tanh", "sigmoid")


class Config(object):
    batch_size = 4
    dropout = 0.1


def refuse(msg):
    print(msg, file=sys.stderr)
    sys.exit(2)


def check_conf(conf):
    """The data route of a conf -- "ark" (``train_scp_path`` / ``valid_scp_path``: Kaldi features somebody made, the reference's
    route) or "wav" (``train_wav_scp`` / ``valid_wav_scp``: '<utt> <path.wav>' lines, the wav.scp of the reference's local/
    scripts) -- or a refusal (status 2, one line on stderr) for a conf with neither pair, both, half of one, or a file that is
    not there.  Before any data is read or the device is touched."""
    ark = [k for k in ("train_scp_path", "valid_scp_path") if conf.get(k)]
    wav = [k for k in ("train_wav_scp", "valid_wav_scp") if conf.get(k)]
    if ark and wav:
        refuse("conf names both data routes (%s and %s): keep the ark pair or the WAV pair" % (", ".join(ark), ", ".join(wav)))
    if not ark and not wav:
        refuse("conf names no training data: set train_scp_path / valid_scp_path (Kaldi features) or train_wav_scp / valid_wav_scp (WAVs)")
    if len(ark or wav) != 2:
        refuse("conf has %s without its partner: a route needs its train and its valid file" % (ark or wav)[0])
    route = "wav" if wav else "ark"
    needed = (ark or wav) + ["train_lab_path", "train_trans_path", "valid_lab_path", "valid_trans_path", "vocab_file"]
    for k in needed:
        if not conf.get(k):
            refuse("conf lacks %s" % k)
        if not os.path.isfile(conf[k]):
            refuse("%s: no file at %s" % (k, conf[k]))
    if route == "wav" and not conf.get("cmvn_path"):
        refuse("the WAV route needs cmvn_path: the global CMVN statistics, computed from the training WAVs and written there if absent")
    return route


def check_mwer(conf):
    """The MWER and fine-tuning keys of a conf: ``mwer_nbest`` (N hypotheses, 2..256; absent or 0: off), ``mwer_weight`` (1.0),
    ``mwer_ctc_weight`` (0.01), ``mwer_beam_width`` (``max(N, 10)``, at most 256) and ``init_model`` (a package of
    ``CTC_Model.save_package`` whose weights the run starts from; with or without ``mwer_nbest``).  Returns ``(N, beam_width)``, N = 0 for
    off, or refuses (status 2, one line on stderr) before any data is read or the device is touched."""
    init = conf.get("init_model")
    if init and not os.path.isfile(init):
        refuse("init_model: no file at %s" % init)
    n = conf.get("mwer_nbest") or 0
    if not n:
        return 0, 0
    if not isinstance(n, int) or not 2 <= n <= 256:
        refuse("mwer_nbest %r: the N-best list of the MWER loss takes 2..256 hypotheses" % (n,))
    beam = conf.get("mwer_beam_width") or max(n, 10)
    if not isinstance(beam, int) or not 1 <= beam <= 256:
        refuse("mwer_beam_width %r: the beam search takes a width of 1..256" % (beam,))
    if n > beam:
        refuse("mwer_nbest %d exceeds mwer_beam_width %d: the search lists at most its beam" % (n, beam))
    if not conf.get("lm_path"):
        refuse("mwer_nbest needs lm_path: the beam search that makes the list reads its bigram table from there")
    if not os.path.isfile(conf["lm_path"]):
        refuse("lm_path: no file at %s" % conf["lm_path"])
    return n, beam


def read_table(path):
    """'<key> <rest of line>' lines -> ordered (key, rest) pairs; keys as SpeechDataset reads them (cut at the first '.')."""
    rows = []
    with open(path, "r") as rf:
        for line in rf:
            if line.strip():
                key, rest = line.strip().split(" ", 1)
                rows.append((key.split(".")[0], rest.strip()))
    return rows


def wav_items(scp_path, lab_path, trans_path):
    """TrainWavLoader items of one split: (utt, WAV path, canonical phones, annotated phones), in the scp's order."""
    scp = read_table(scp_path)
    labels, trans = (dict(read_table(p)) for p in (lab_path, trans_path))
    for utt, _ in scp:
        if utt not in labels or utt not in trans:
            refuse("%s: no %s line for %s" % (scp_path, "label" if utt not in labels else "transcript", utt))
    return [(utt, path, trans[utt], labels[utt]) for utt, path in scp]


def wav_cmvn(items, path, batch_size):
    """The (scale, offset) pair of the global CMVN file at ``path``; a file that is not there is first computed from the training
    WAVs on the GPU (``fbank.cmvn_stats``) and written -- the compute-cmvn-stats step of AA/steps/make_feat.sh:24-39."""
    from ..utils import fbank
    if not os.path.exists(path):
        def batches():
            for start in range(0, len(items), batch_size):
                read = [fbank.read_wav(it[1], with_format=True) for it in items[start:start + batch_size]]
                wavs = [fbank.quantize_pcm16(x) if rate == fbank.SAMPLE_RATE and not pcm16 else x for x, rate, pcm16 in read]
                if all(rate == fbank.SAMPLE_RATE for _, rate, _ in read):
                    for w in wavs:
                        yield w
                else:
                    yield fbank.resample_batch(wavs, [rate for _, rate, _ in read])
        stats = fbank.cmvn_stats(batches(), batch_size=batch_size)
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        fbank.write_cmvn_stats(path, stats)
        print("CMVN statistics of %d training utterances (%d frames) written to %s" % (len(items), int(stats[0, -1]), path))
    return fbank.cmvn_scale_offset(fbank.read_cmvn_stats(path))


def main(conf):
    """AA/steps/train_ctc.py:111-291 over run_epoch / LrSchedule / build_training: seeds, Vocab, the two loaders, the model from the
    conf's rnn_* and CNN keys, the epoch loop with the reference's printed lines, the best-accuracy state into
    ``checkpoint_dir/exp_name/ctc_best_model.pkl`` -- the checkpoint ``infer.load_model`` reads.  New conf keys: ``train_wav_scp`` /
    ``valid_wav_scp`` + ``cmvn_path`` (the WAV route, ``TrainWavLoader``), ``speed_perturb`` (a list of factors for it),
    ``train_precision`` ("f32", "bf16x3" or "f32x6"), ``init_model`` and the ``mwer_*`` keys (``check_mwer``: fine-tuning towards the
    phoneme error rate with ``train.MWERLoss`` on the training epochs; needs ``lm_path``, reads ``lm_alpha``).  Every rank reads the whole data: sharding it is not built."""
    route = check_conf(conf)
    mwer_nbest, mwer_beam = check_mwer(conf)
    import ast
    import time

    import numpy as np
    import torch.nn as nn
    from ..models.model_ctc import CTC_Model
    from ..utils.data_loader import SpeechDataLoader, SpeechDataset, TrainWavLoader, Vocab
    opts = Config()
    for k, v in conf.items():
        setattr(opts, k, v)
        print('{:50}:{}'.format(k, v))
    if opts.rnn_type not in SUPPORTED_RNN or opts.activation_function not in SUPPORTED_ACTIVATE:
        refuse("rnn_type must be one of %s and activation_function one of %s" % (SUPPORTED_RNN, SUPPORTED_ACTIVATE))
    precision = getattr(opts, "train_precision", None)
    if precision is not None and precision not in ("f32", "bf16x3", "f32x6"):
        refuse("train_precision %r: f32, bf16x3 or f32x6" % (precision,))

    device = torch.device('cuda:0') if opts.use_gpu else torch.device('cpu')
    torch.manual_seed(opts.seed)
    np.random.seed(opts.seed)
    if opts.use_gpu:
        torch.cuda.manual_seed(opts.seed)

    vocab = Vocab(opts.vocab_file)
    n_downsample = getattr(opts, "n_downsample", 2)
    if route == "ark":
        for k in ("train_scp_path", "train_lab_path", "train_trans_path", "valid_scp_path", "valid_lab_path", "valid_trans_path"):
            print(getattr(opts, k))
        train_dataset = SpeechDataset(vocab, opts.train_scp_path, opts.train_lab_path, opts.train_trans_path, opts, True)
        dev_dataset = SpeechDataset(vocab, opts.valid_scp_path, opts.valid_lab_path, opts.valid_trans_path, opts)
        train_loader = SpeechDataLoader(train_dataset, batch_size=opts.batch_size, shuffle=opts.shuffle_train, num_workers=opts.num_workers)
        dev_loader = SpeechDataLoader(dev_dataset, batch_size=opts.batch_size, shuffle=False, num_workers=opts.num_workers)
    else:
        for k in ("train_wav_scp", "train_lab_path", "train_trans_path", "valid_wav_scp", "valid_lab_path", "valid_trans_path"):
            print(getattr(opts, k))
        if getattr(opts, "left_ctx", 0) != 0:
            refuse("the WAV route stacks right context only (left_ctx: 0, as every conf of the reference has it)")
        train_items = wav_items(opts.train_wav_scp, opts.train_lab_path, opts.train_trans_path)
        dev_items = wav_items(opts.valid_wav_scp, opts.valid_lab_path, opts.valid_trans_path)
        cmvn = wav_cmvn(train_items, opts.cmvn_path, opts.batch_size)
        geometry = dict(cmvn=cmvn, right_ctx=opts.right_ctx, n_skip_frame=opts.n_skip_frame, n_downsample=n_downsample)
        train_loader = TrainWavLoader(train_items, vocab, opts.batch_size, train=True, shuffle=opts.shuffle_train,
                                      speeds=getattr(opts, "speed_perturb", None), **geometry)
        dev_loader = TrainWavLoader(dev_items, vocab, opts.batch_size, train=False, shuffle=False, **geometry)

    rnn_type = getattr(nn, opts.rnn_type.split(".", 1)[1])
    rnn_param = {"rnn_input_size": opts.rnn_input_size, "rnn_hidden_size": opts.rnn_hidden_size, "rnn_layers": opts.rnn_layers,
                 "rnn_type": rnn_type, "bidirectional": opts.bidirectional, "batch_norm": opts.batch_norm}
    num_class = vocab.n_words
    opts.output_class_dim = vocab.n_words
    channel, kernel_size, stride, padding, pooling = (ast.literal_eval(getattr(opts, k)) for k in
                                                      ("channel", "kernel_size", "stride", "padding", "pooling"))
    activation = {"relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}[opts.activation_function]
    cnn_param = {"batch_norm": opts.batch_norm, "activate_function": activation,
                 "layer": [[channel[n], kernel_size[n], stride[n], padding[n], pooling[n] if pooling is not None else None]
                           for n in range(opts.layers)]}
    model = CTC_Model(add_cnn=opts.add_cnn, cnn_param=cnn_param, rnn_param=rnn_param, num_class=num_class, drop_out=opts.drop_out)
    if getattr(opts, "init_model", None):                    # fine-tuning: the weights of an earlier run's package
        model.load_state_dict(torch.load(opts.init_model, map_location="cpu", weights_only=False)["state_dict"])
        print("Initial weights from %s" % opts.init_model)
    model = model.to(device)
    if precision is not None:
        model.train_precision = precision
    print("Number of parameters %d" % sum(p.numel() for p in model.parameters()))
    for idx, m in enumerate(model.children()):
        print(idx, m)

    params = {'num_epoches': opts.num_epoches, 'end_adjust_acc': opts.end_adjust_acc, 'mel': opts.mel, 'seed': opts.seed,
              'decay': opts.lr_decay, 'learning_rate': opts.init_lr, 'weight_decay': opts.weight_decay, 'batch_size': opts.batch_size,
              'feature_type': opts.feature_type, 'n_feats': opts.feature_dim}
    print(params)
    loss_fn, optimizer = build_training(model, init_lr=opts.init_lr, weight_decay=opts.weight_decay)
    train_loss_fn = loss_fn
    if mwer_nbest:       # the training epochs alone: the validation epoch keeps the CTC loss, so dev_loss, the schedule and the best checkpoint keep their meaning
        from ..train import MWERLoss
        from ..utils.ctcDecoder import BeamDecoder
        decoder = BeamDecoder(vocab.index2word, beam_width=mwer_beam, lm_path=opts.lm_path, lm_alpha=getattr(opts, "lm_alpha", 0.01))
        train_loss_fn = MWERLoss(decoder, mwer_nbest, ctc_weight=getattr(opts, "mwer_ctc_weight", 0.01), mwer_weight=getattr(opts, "mwer_weight", 1.0))
        print("MWER training: %d-best of beam %d, mwer_weight %g, ctc_weight %g" % (mwer_nbest, mwer_beam, train_loss_fn.mwer_weight, train_loss_fn.ctc_weight))
    schedule = LrSchedule(model, optimizer, opts.init_lr, opts.lr_decay, opts.end_adjust_acc, opts.num_epoches)
    start_time = time.time()
    loss_results, dev_loss_results, dev_cer_results = [], [], []
    while schedule.begin_epoch():
        count = schedule.count
        print("Start training epoch: %d, learning_rate: %.5f" % (count, schedule.learning_rate))
        _, loss = run_epoch(count, model, train_loader, train_loss_fn, device, optimizer=optimizer, print_every=opts.verbose_step, is_training=True)
        loss_results.append(loss)
        acc, dev_loss = run_epoch(count, model, dev_loader, loss_fn, device, optimizer=None, print_every=opts.verbose_step, is_training=False)
        dev_loss_results.append(dev_loss)
        dev_cer_results.append(acc)
        schedule.end_epoch(acc, dev_loss)
        print("adjust_rate_count:" + str(schedule.printed_count) + ' adjust_time:' + str(schedule.printed_time))
        print("epoch %d done, cv acc is: %.4f, time_used: %.4f minutes" % (count, acc, (time.time() - start_time) / 60))
        print('dev loss:', dev_loss, 'loss_best:', schedule.loss_best)
        print('\n')
    print("End training, best dev loss is: %.4f, acc is: %.4f" % (schedule.loss_best, schedule.acc_best))
    schedule.finish()
    save_dir = os.path.join(opts.checkpoint_dir, opts.exp_name)
    os.makedirs(save_dir, exist_ok=True)
    best_path = os.path.join(save_dir, 'ctc_best_model.pkl')
    params['epoch'] = schedule.count
    torch.save(CTC_Model.save_package(model, optimizer=optimizer, epoch=params, loss_results=loss_results, dev_loss_results=dev_loss_results,
                                      dev_cer_results=dev_cer_results), best_path)
    return best_path


def cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="train the CNN + BiLSTM + attention CTC model on the MI355X path")
    ap.add_argument("--conf", default="conf/ctc_config.yaml", help="conf file with the arguments of the model and the training")
    args = ap.parse_args(argv)
    import yaml
    try:
        with open(args.conf, "r") as f:
            conf = yaml.safe_load(f)
    except (OSError, yaml.YAMLError):
        print("No input config or config file missing, please check.")
        sys.exit(1)
    if not isinstance(conf, dict):
        refuse("%s: not a mapping of conf keys" % args.conf)
    main(conf)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
