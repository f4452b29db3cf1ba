"""Drop-in for the reference's ``models/model_ctc.py`` (AA/models/model_ctc.py).

Same class names, constructor arguments, ``state_dict`` keys, ``forward(x, x1[, visualize])``
signature and return layout ([T/2, B, C] log-probabilities) as the reference, so that
``from models.model_ctc import *`` in AA/infer.py:24 can be pointed here unchanged.  The torch
modules below are parameter containers only (they give the 61 reference key names and make
``load_state_dict`` / ``.to()`` work); the arithmetic of ``forward`` runs in hand-written gfx950
kernels behind the C ABI of libmdd_hip.so (include/mdd_hip.h): eval mode through mdd_forward, train mode (BatchNorm on batch
statistics, dropout, differentiable w.r.t. every parameter) through mdd_train_forward / mdd_train_backward (train.py).

AA/infer.py also relies on this module re-exporting ``math`` (infer.py:342) -- kept, together with
the other names the reference module exposes through ``import *``.
"""
import math  # noqa: F401  (re-exported on purpose)
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401

from .. import _lib
from ..hip_model import HipModel


class _EditDistance(object):
    """Stand-in for the third-party ``editdistance`` module the reference imports as ``ed``
    (model_ctc.py:7); only ``ed.eval`` is used (model_ctc.py:240)."""

    @staticmethod
    def eval(a, b):
        a, b = list(a), list(b)
        prev = list(range(len(b) + 1))
        for i, ca in enumerate(a, 1):
            row = [i]
            for j, cb in enumerate(b, 1):
                row.append(min(row[j - 1] + 1, prev[j] + 1, prev[j - 1] + (ca != cb)))
            prev = row
        return prev[len(b)]


ed = _EditDistance()


class BatchRNN(nn.Module):
    """Parameter container with the reference's names: ``batch_norm.*`` (layers > 0) and
    ``rnn.weight_{ih,hh}_l0[_reverse]`` (model_ctc.py:15-34)."""

    def __init__(self, input_size, hidden_size, rnn_type=nn.LSTM, bidirectional=False, batch_norm=True,
                 dropout=0.1, skip=False):
        super(BatchRNN, self).__init__()
        if skip:
            raise NotImplementedError("skip projections are never enabled by the reference recipe")
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bidirectional
        self.batch_norm = nn.BatchNorm1d(input_size) if batch_norm else None
        self.rnn = rnn_type(input_size=input_size, hidden_size=hidden_size, bidirectional=bidirectional, bias=False)


class LayerCNN(nn.Module):
    """Parameter container: ``conv.*`` + ``batch_norm.*`` (model_ctc.py:51-71)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride, padding, pooling_size=None,
                 activation_function=nn.ReLU, batch_norm=True, dropout=0.1):
        super(LayerCNN, self).__init__()
        self.conv = nn.Conv2d(in_channel, out_channel, kernel_size=kernel_size, stride=stride, padding=padding)
        self.batch_norm = nn.BatchNorm2d(out_channel) if batch_norm else None
        self.geometry = (tuple(kernel_size), tuple(stride), tuple(padding), pooling_size)


class CTC_Model(nn.Module):
    # models/cnn_rnn.py derives the reference's CTC-only baseline model (CRC/models/cnn_rnn.py) from this class by setting the flag: no
    # embedding, text encoder or score; the classifier on the 2H outputs of the last BiLSTM; a handle of mdd_create_ctc
    _ctc_only = False

    def __init__(self, add_cnn=False, cnn_param=None, rnn_param=None, num_class=39, drop_out=0.1):
        super(CTC_Model, self).__init__()
        self.add_cnn = add_cnn
        self.cnn_param = cnn_param
        if rnn_param is None or type(rnn_param) != dict:
            raise ValueError("rnn_param need to be a dict to contain all params of rnn!")
        self.rnn_param = rnn_param
        self.num_class = num_class
        self.num_directions = 2 if rnn_param["bidirectional"] else 1
        self.drop_out = drop_out
        feat = rnn_param["rnn_input_size"]
        width = feat
        if add_cnn:
            layers = []
            for n, (chan, ksz, stride, pad, pool) in enumerate(cnn_param["layer"]):
                layers.append(("%d" % n, LayerCNN(chan[0], chan[1], ksz, stride, pad, pool,
                                                  activation_function=cnn_param["activate_function"],
                                                  batch_norm=cnn_param["batch_norm"], dropout=drop_out)))
                width = int(math.floor((width + 2 * pad[1] - ksz[1]) / stride[1]) + 1)
            self.conv = nn.Sequential(OrderedDict(layers))
            width *= cnn_param["layer"][-1][0][1]
        H = rnn_param["rnn_hidden_size"]
        rnns = [("0", BatchRNN(width, H, rnn_type=rnn_param["rnn_type"], bidirectional=rnn_param["bidirectional"],
                               dropout=drop_out, batch_norm=False))]
        for i in range(rnn_param["rnn_layers"] - 1):
            rnns.append(("%d" % (i + 1), BatchRNN(self.num_directions * H, H, rnn_type=rnn_param["rnn_type"],
                                                  bidirectional=rnn_param["bidirectional"], dropout=drop_out,
                                                  batch_norm=rnn_param["batch_norm"])))
        self.rnns = nn.Sequential(OrderedDict(rnns))
        if not self._ctc_only:
            self.embeds = nn.Embedding(44, 512)                                       # model_ctc.py:149
            self.lstm_embeds = nn.LSTM(512, H, batch_first=True, bidirectional=True)  # :150
            self.score = nn.Linear(H * 2, H * 2, bias=False)                          # :151
        fc_in = self.num_directions * H * (1 if self._ctc_only else 2)   # cat(X, context), or X alone (cnn_rnn.py:140-142)
        if rnn_param["batch_norm"]:
            self.fc = nn.Sequential(nn.BatchNorm1d(fc_in), nn.Linear(fc_in, num_class, bias=False))
        else:
            self.fc = nn.Linear(fc_in, num_class, bias=False)
        self.log_softmax = nn.LogSoftmax(dim=-1)
        self._hip = None            # the decode handle (hip_model.HipModel), on the device of the last eval forward's inputs
        self._dirty = True          # the module's weights are not the handle's
        self._taps = False
        self.strict_errors = True   # raise IndexError for bad canonical ids synchronously, like nn.Embedding
        self._dropout_masks = None  # tests: the reference's own dropout masks (one uint8 tensor per site, mdd_hip.h); None = drawn
        self.train_precision = None  # train mode: None = library default (exact fp32, or MDD_TRAIN_PRECISION), "f32", "bf16x3" (flagged variant) or "f32x6" (reference width on the bf16 matrix cores)

    # ------------------------------------------------------------------ library plumbing
    def _check_supported(self):
        p, c = self.rnn_param, self.cnn_param
        ok = (self.add_cnn and p["bidirectional"] and p["batch_norm"] and c["batch_norm"] and p["rnn_type"] is nn.LSTM
              and len(c["layer"]) == 2
              and [l.geometry for l in self.conv] == [((3, 3), (1, 2), (1, 1), None), ((3, 3), (2, 2), (1, 1), None)]
              and c["layer"][0][0][0] == 1 and c["layer"][0][0][1] == c["layer"][1][0][0] == c["layer"][1][0][1])
        if not ok:
            raise NotImplementedError("libmdd_hip implements the architecture of conf/ctc_config.*.yaml "
                                      "(2x conv k3 s(1,2),(2,2) p1 + BN, BiLSTM + BN); got something else")

    def _config(self):
        return _lib.MddConfig(feat=self.rnn_param["rnn_input_size"], hidden=self.rnn_param["rnn_hidden_size"],
                              layers=self.rnn_param["rnn_layers"], num_class=self.num_class,
                              channels=self.cnn_param["layer"][0][0][1],
                              emb_rows=0 if self._ctc_only else self.embeds.num_embeddings,
                              emb_dim=0 if self._ctc_only else self.embeds.embedding_dim, bn_eps=self.fc[0].eps)

    def _sync_weights(self, index):
        """The handle on cuda:``index`` with the module's weights as they are now; inputs on another device get a new handle there."""
        if self._hip is None or self._hip.device.index != index:
            self._check_supported()
            if self._hip is not None:
                self._hip.close()
            self._hip = HipModel.from_config(self._config(), self._ctc_only, index)
            self._dirty = True
        if self._dirty:
            self._hip.load_state_dict(self.state_dict())
            self._dirty = False

    def _on_device(self, x, taps):
        """x as the kernels take it (host features: on the current device), that device's handle up to date and, on request, its taps on."""
        xd = _lib.to_gpu(x, torch.float32)
        B, T, Fdim = xd.shape
        if Fdim != self.rnn_param["rnn_input_size"]:
            raise RuntimeError("expected feature size %d, got %d" % (self.rnn_param["rnn_input_size"], Fdim))
        with torch.cuda.device(xd.device):
            self._sync_weights(xd.device.index)
        if taps:
            self._hip.enable_taps(True)
        return xd

    def load_state_dict(self, *args, **kwargs):
        self._dirty = True
        return super(CTC_Model, self).load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._dirty = True
        return super(CTC_Model, self)._apply(fn, *args, **kwargs)

    def mark_weights_changed(self):
        """Call after editing parameters in place."""
        self._dirty = True

    def enable_taps(self, on=True):
        self._taps = bool(on)
        if self._hip is not None:
            self._hip.enable_taps(on)

    def tap(self, name):
        """Stage output of the last forward as a torch tensor (copy) on the handle's device: conv1, rnn<i>, text, key."""
        if self._hip is None:
            raise KeyError(name)
        with torch.cuda.device(self._hip.device):
            return self._hip.tap(name)

    # ------------------------------------------------------------------ the reference API
    def forward(self, x, x1, visualize=False):
        """x: [B, T, F] float stacked features (T even); x1: [B, L] long canonical phoneme ids.
        Returns log-probabilities [T/2, B, num_class] on x's device (model_ctc.py:160-223)."""
        if not self.add_cnn:
            print("error")          # model_ctc.py:224-225
            return None
        if self.training and self._ctc_only:
            raise NotImplementedError("CTC-only training is not built: the training step (mdd_train_*) covers the attention model; "
                                      "call .eval() for the decode forward")
        _lib.require_gpu()
        if self.training:      # BatchNorm on batch statistics, Dropout(drop_out) behind each LayerCNN / BatchRNN; differentiable
            if visualize:
                raise NotImplementedError("visualize=True is an eval-mode facility here")
            from ..train import model_forward_train
            return model_forward_train(self, x, x1, masks=getattr(self, "_dropout_masks", None))
        xd = self._on_device(x, self._taps or visualize)
        idd = None if self._ctc_only else x1.to(xd.device, torch.int64).contiguous()   # (the CTC-only forward never reads x1: cnn_rnn.py:147)
        with torch.cuda.device(xd.device):
            out = self._hip.forward(xd, idd, sync_errors=self.strict_errors).to(x.device)
            if visualize:
                B, T, ch = xd.shape[0], xd.shape[1], self.cnn_param["layer"][-1][0][1]
                seq = self._hip.tap("conv1").view(T // 2, B, -1)
                cnn = seq.view(T // 2, B, ch, -1).permute(1, 2, 0, 3).contiguous()
                return out, [x, cnn.to(x.device), seq.to(x.device), out]
        return out

    def forward_candidates(self, x, candidates):
        """Several canonical candidates per utterance on one acoustic pass (no reference counterpart; mdd_forward_candidates).
        x: [B, T, F] as ``forward`` takes it; candidates: a list of K LongTensors [B, L_k], host or device, each one a canonical batch as
        ``forward``'s x1 (padded to its own longest, as the reference's collate pads a batch).  Returns a list of K tensors [T/2, B, num_class]
        on x's device: entry k is what ``forward(x, candidates[k])`` returns -- bit for bit wherever B and K*B rows run the same kernels
        (include/mdd_hip.h at mdd_forward_candidates: hidden 384 up to K*B = 1024, any geometry while K*B <= 128), within the parity tolerance
        elsewhere.  The conv front end and the BiLSTM layers run once.  Eval mode only."""
        if self._ctc_only:
            raise NotImplementedError("forward_candidates: the CTC-only model has no canonical side -- its posteriors do not depend on the "
                                      "canonical phones, so one forward serves every candidate")
        if self.training:
            raise NotImplementedError("forward_candidates is an eval-mode facility: call .eval() first")
        if not self.add_cnn:
            print("error")
            return None
        candidates = list(candidates)
        if not candidates:
            raise ValueError("forward_candidates: at least one candidate batch is needed")
        _lib.require_gpu()
        xd = self._on_device(x, self._taps)
        B, dev = xd.shape[0], xd.device
        K, L = len(candidates), max(int(c.shape[1]) for c in candidates)
        ids = torch.zeros((K, B, L), dtype=torch.int64, device=dev)
        for k, c in enumerate(candidates):
            if c.dim() != 2 or c.shape[0] != B or c.shape[1] < 1:
                raise ValueError("forward_candidates: candidate %d is %s, expected [%d, L >= 1]" % (k, tuple(c.shape), B))
            ids[k, :, :c.shape[1]] = c.to(dev, torch.int64)
        canon = torch.tensor([int(c.shape[1]) for c in candidates], dtype=torch.int32).repeat_interleave(B).to(dev)
        with torch.cuda.device(dev):
            out = self._hip.forward_candidates(xd, ids, canon=canon, sync_errors=self.strict_errors)
        return [out[k].to(x.device) for k in range(K)]

    def compute_wer(self, index, input_sizes, targets, target_sizes):
        """Greedy collapse + edit distance on host index arrays (model_ctc.py:227-244)."""
        errs = toks = 0
        for i in range(len(index)):
            label = targets[i][:target_sizes[i]]
            frames = index[i][:input_sizes[i]]
            pred = [frames[j] for j in range(len(frames))
                    if frames[j] != 0 and (j == 0 or frames[j] != frames[j - 1])]
            errs += ed.eval(label, pred)
            toks += len(label)
        return errs, toks

    def add_weights_noise(self):
        """model_ctc.py:246-249: draws N(0, 0.075) noise per parameter and binds the sum to a LOCAL name -- the parameters are left
        as they are; what the call does observably is advance the generator, which is kept."""
        for param in self.parameters():
            param.data.new(param.size()).normal_(0, 0.075)

    @staticmethod
    def save_package(model, optimizer=None, decoder=None, epoch=None, loss_results=None, dev_loss_results=None,
                     dev_cer_results=None):
        """Checkpoint dict with the reference's keys (model_ctc.py:251-271)."""
        package = {"rnn_param": model.rnn_param, "add_cnn": model.add_cnn, "cnn_param": model.cnn_param,
                   "num_class": model.num_class, "_drop_out": model.drop_out, "state_dict": model.state_dict()}
        for key, val in (("optim_dict", optimizer.state_dict() if optimizer is not None else None),
                         ("decoder", decoder), ("epoch", epoch)):
            if val is not None:
                package[key] = val
        if loss_results is not None:
            package.update(loss_results=loss_results, dev_loss_results=dev_loss_results, dev_cer_results=dev_cer_results)
        return package
