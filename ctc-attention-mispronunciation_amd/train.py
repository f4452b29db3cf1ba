"""Training-side plumbing over the C ABI (include/mdd_hip.h, "SURVEY 8(f) #3"): the pieces `run_epoch` of the reference uses
(AA/steps/train_ctc.py:28-105) -- train-mode ``model(inputs, trans)``, ``nn.CTCLoss(reduction='sum')``, ``loss.backward()``,
``optimizer.step()`` -- as torch.autograd Functions and an optimizer whose arithmetic runs in libmdd_hip.so.

* ``TrainHandle``   one mdd_train_ws: tensor table, forward / backward on raw device pointers.
* ``model_forward_train(model, x, x1, masks=None)``   what ``CTC_Model.forward`` calls in train mode; differentiable w.r.t. every
  parameter (autograd Function; the model's BatchNorm running statistics are updated in place, as nn.BatchNorm does).
* ``CTCLoss``       drop-in for ``nn.CTCLoss`` (same constructor / call signature, train_ctc.py:72,186) over mdd_ctc_loss.
* ``MWERLoss``      the expected number of phoneme errors over the beam search's N-best list, interpolated with the CTC loss; called like
  ``CTCLoss`` (mdd_beam_nbest -> mdd_ctc_nbest -> mdd_nbest_mbr -> mdd_nbest_risk -> mdd_ctc_nbest_grad); torch only
  weights and adds the two gradient tensors and sums the per-utterance scalars.
* ``Adam``          ``torch.optim.Adam``-compatible optimizer (lr, betas, eps, weight_decay, state_dict) over mdd_adam_step.
PyTorch supplies device memory, streams and the autograd tape; no torch operator computes anything on this path.
"""
import ctypes as C

import torch

from . import _lib


class TrainHandle(object):
    def __init__(self, cfg, device_index):
        _lib.require_gpu()
        L = _lib.lib()
        self.device_index = device_index
        self.handle = _lib.new_handle(L.mdd_train_create, cfg, device_index)
        n = L.mdd_train_num_tensors(self.handle)
        self.keys, self.numel, self.is_buffer = [], [], []
        buf = C.create_string_buffer(128)
        for i in range(n):
            ne, ib = C.c_int64(0), C.c_int32(0)
            _lib.check(L.mdd_train_tensor_info(self.handle, i, buf, 128, C.byref(ne), C.byref(ib)))
            self.keys.append(buf.value.decode()); self.numel.append(ne.value); self.is_buffer.append(bool(ib.value))
        self.n_masks = L.mdd_train_num_masks(self.handle)

    def mask_shapes(self, geom_channels, hidden, B, T, W1, W2):
        return [(B, geom_channels, T, W1), (B, geom_channels, T // 2, W2)] + [(T // 2, B, 2 * hidden)] * (self.n_masks - 2)

    _ptr_array = staticmethod(_lib.ptr_array)

    def forward(self, tensors, x, x1, masks, seed, p_drop):
        B, T, _ = x.shape
        out = torch.empty((T // 2, B, self._num_class(tensors)), dtype=torch.float32, device=x.device)
        assert masks is None or len(masks) == self.n_masks
        marr = None if masks is None else _lib.ptr_array(masks)
        _lib.check(_lib.lib().mdd_train_forward(self.handle, _lib.ptr_array(tensors), _lib.ptr(x), B, T, _lib.ptr(x1), x1.shape[1], marr,
                                                C.c_uint64(seed), C.c_float(p_drop), _lib.ptr(out), _lib.current_stream_ptr()))
        return out

    def _num_class(self, tensors):
        return tensors[self.keys.index("fc.1.weight")].shape[0]

    def backward(self, tensors, dlogp, grads):
        _lib.check(_lib.lib().mdd_train_backward(self.handle, _lib.ptr_array(tensors), _lib.ptr(dlogp), _lib.ptr_array(grads),
                                                 _lib.current_stream_ptr()))

    def sync(self):
        _lib.raise_device_error(_lib.lib().mdd_train_sync, self.handle)

    def close(self):
        if self.handle:
            _lib.lib().mdd_train_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class _TrainForward(torch.autograd.Function):
    """logp = CTC_Model.forward(x, x1) in train mode; backward hands every parameter its gradient."""

    @staticmethod
    def forward(ctx, handle, x, x1, masks, seed, p_drop, all_tensors, *params):
        # all_tensors: the state tensors in the handle's order (parameters AND running-statistics buffers); params are the
        # differentiable ones among them (passed separately so that autograd tracks them)
        ctx.handle, ctx.all_tensors, ctx.keep = handle, all_tensors, (x, x1, masks)
        with torch.cuda.device(x.device):
            return handle.forward(all_tensors, x, x1, masks, seed, p_drop)

    @staticmethod
    def backward(ctx, dlogp):
        h = ctx.handle
        dev = dlogp.device
        grads = [None if h.is_buffer[i] else torch.empty(h.numel[i], dtype=torch.float32, device=dev) for i in range(len(h.keys))]
        with torch.cuda.device(dev):
            h.backward(ctx.all_tensors, dlogp.contiguous(), grads)
        out = [g.view_as(t) for g, t, b in zip(grads, ctx.all_tensors, h.is_buffer) if not b]
        return (None, None, None, None, None, None, None) + tuple(out)


def model_forward_train(model, x, x1, masks=None, seed=None):
    """Train-mode forward of the drop-in CTC_Model through libmdd_hip (called by CTC_Model.forward when model.training)."""
    xd = _lib.to_gpu(x, torch.float32)
    dev, index = xd.device, xd.device.index
    idd = x1.to(dev, torch.int64).contiguous()
    h = getattr(model, "_train_handle", None)
    if h is None or h.device_index != index:
        h = TrainHandle(model._config(), index)
        model._train_handle = h
    want = getattr(model, "train_precision", None)          # None: the library default (exact fp32, or MDD_TRAIN_PRECISION)
    if want is not None and want != getattr(h, "precision", None):
        if want not in _lib.PRECISIONS:
            raise ValueError("train_precision %r: expected one of %s" % (want, ", ".join(repr(k) for k in _lib.PRECISIONS)))
        _lib.check(_lib.lib().mdd_train_set_precision(h.handle, _lib.PRECISIONS[want]))    # the large contractions: exact fp32 | flagged split-bf16 x3 | f32x6
        h.precision = want
    sd = dict(model.named_parameters())
    sd.update(dict(model.named_buffers()))
    tensors = []
    for key, ne in zip(h.keys, h.numel):
        t = sd[key]
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("train-mode forward needs the model on %s in float32 (model.to(%r)); %s is on %s" % (dev, str(dev), key, t.device))
        assert t.numel() == ne, (key, t.numel(), ne)
        tensors.append(t)
    params = [t for t, b in zip(tensors, h.is_buffer) if not b]
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())        # consumes torch's CPU generator: reproducible under torch.manual_seed
    if masks is not None:
        masks = [m.to(dev, torch.uint8).contiguous() for m in masks]
    out = _TrainForward.apply(h, xd, idd, masks, seed, float(model.drop_out), tensors, *params)
    for name, buf in model.named_buffers():                        # nn.BatchNorm counts its batches
        if name.endswith("num_batches_tracked"):
            buf += 1
    if getattr(model, "strict_errors", True):
        h.sync()
    model.mark_weights_changed()                                   # the eval path's packed weight copies are stale now
    return out if x.device == dev else out.to(x.device)


class _CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank):
        from .hip_model import ctc_loss
        nll, grad = ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=blank, want_grad=log_probs.requires_grad)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0))
        return nll

    @staticmethod
    def backward(ctx, gnll):
        (grad,) = ctx.saved_tensors
        return grad * gnll.view(1, -1, 1), None, None, None, None


class CTCLoss(torch.nn.Module):
    """``nn.CTCLoss`` over the gfx950 lattice kernel (mdd_ctc_loss): log_probs [T,B,C] (cuda, float32), padded 2-D or
    concatenated 1-D targets, input / target lengths -- same call and reductions as torch (train_ctc.py:72,186 uses
    reduction='sum', blank 0)."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super(CTCLoss, self).__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError("%s is not a valid value for reduction" % reduction)
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        dev = log_probs.device
        il = torch.as_tensor(input_lengths, dtype=torch.int64)
        tl = torch.as_tensor(target_lengths, dtype=torch.int64)
        tg = _padded_targets(targets, tl)                           # concatenated targets -> padded [B, Lmax]
        nll = _CTCLossFn.apply(log_probs, tg.to(dev), il.to(dev), tl.to(dev), self.blank)
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        return (nll / tl.to(dev).clamp(min=1).to(nll.dtype)).mean()


def _padded_targets(targets, target_lengths):
    """Targets as a padded 2-D int64 tensor [B, Lmax] (concatenated 1-D targets are cut at the lengths, as ``CTCLoss.forward`` does)."""
    tl = torch.as_tensor(target_lengths, dtype=torch.int64)
    tg = torch.as_tensor(targets)
    if tg.dim() != 1:
        return tg
    B, Lm = tl.numel(), int(tl.max()) if tl.numel() else 0
    pad = torch.zeros((B, max(Lm, 1)), dtype=torch.int64)
    off, tgc = 0, tg.cpu()
    for b in range(B):
        n = int(tl[b])
        pad[b, :n] = tgc[off:off + n]
        off += n
    return pad


class _MWERLossFn(torch.autograd.Function):
    """The whole chain on ``log_probs.detach()``; the gradient is made in ``forward`` and scaled by the upstream scalar in ``backward``."""

    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, mod):
        from . import hip_model
        lp = log_probs.detach()
        want_grad = log_probs.requires_grad
        T, B, Cn = lp.shape
        blank, N = mod.blank, mod.nbest
        lens = input_lengths.to(lp.device, torch.int32).clamp(0, T)
        nll, grad_ctc = hip_model.ctc_loss(lp, targets, input_lengths, target_lengths, blank=blank, want_grad=want_grad)
        # 1. the list; its longest hypothesis bounds the lattices (one host synchronisation: a tight bound is a quarter of the scan's work)
        ids, nids, status, _ = mod.decoder.decode_nbest_ids(lp, lens, N)
        pitch = ids.shape[2]
        width = max(int(nids.max().item()), 1)
        one_launch = hip_model.ctc_nbest_fits(T, Cn, width)
        fused = not mod.per_rank and one_launch and hip_model.ctc_nbest_grad_fits(T, Cn, width)
        per_rank = None
        if not one_launch or (want_grad and not fused):
            per_rank = [hip_model.ctc_loss(lp, ids[n, :, :width], lens, nids[n], blank=blank, want_grad=want_grad) for n in range(N)]
        # 2. exact log-likelihoods, fp64 as the kernel leaves them (the per-rank route has the same values rounded through fp32)
        if one_launch:
            loglik = hip_model.ctc_nbest(lp, lens, ids, nids, blank=blank, max_len=width)
        else:
            loglik = -torch.stack([r[0] for r in per_rank]).double()
        # 3. edit distances to the annotated phones (uniform weights: only ref_dist is used)
        ref = targets.to(lp.device, torch.int32)
        L_mbr = max(pitch, ref.shape[1], 1)
        if L_mbr > hip_model.MBR_MAX_LEN:
            raise ValueError("MWERLoss: a sequence of %d ids; mdd_nbest_mbr takes at most %d" % (L_mbr, hip_model.MBR_MAX_LEN))
        mbr_ids = ids if L_mbr == pitch else torch.nn.functional.pad(ids, (0, L_mbr - pitch))
        uniform = torch.full((N, B), 1.0 / N, dtype=torch.float64, device=lp.device)
        ref_dist = hip_model.nbest_mbr(mbr_ids, nids, status, uniform, Cn, max_len=L_mbr, ref=ref, ref_len=target_lengths)[4]
        # 4. posteriors, risk, coefficients
        post, risk, coef, flag = hip_model.nbest_risk(loglik, ref_dist, status)
        # 5. the gradient of the risk
        grad = None
        if want_grad:
            if fused:
                grad, gflag, _ = hip_model.ctc_nbest_grad(lp, lens, ids, nids, coef, blank=blank, max_len=width)
            else:
                grad = torch.zeros_like(lp)
                gflag = torch.zeros_like(flag)
                for n, (nll_n, g_n) in enumerate(per_rank):
                    live = coef[n] != 0
                    gflag = torch.where(live & ~torch.isfinite(nll_n), torch.ones_like(gflag), gflag)
                    k = coef[n].float().view(1, B, 1)
                    grad = grad + torch.where(live.view(1, B, 1), k * g_n, torch.zeros_like(g_n))
            flag = torch.maximum(flag, gflag)
            flagged = (flag != 0).view(1, B, 1)
            grad = torch.where(flagged, torch.zeros_like(grad), grad) * mod.mwer_weight + grad_ctc * mod.ctc_weight
        risk = torch.where(flag != 0, torch.zeros_like(risk), risk)
        mod.last = dict(ids=ids, nids=nids, status=status, loglik=loglik, ref_dist=ref_dist, post=post, risk=risk, coef=coef, flag=flag,
                        nll=nll, fused=fused)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0))
        return (mod.mwer_weight * risk.sum() + mod.ctc_weight * nll.double().sum()).float()

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None, None, None, None


class MWERLoss(torch.nn.Module):
    """Minimum-word-error-rate training (Prabhavalkar et al. 2018) on phonemes: the expected number of phoneme errors over the N-best
    list the beam search returns, interpolated with the CTC loss --
    ``mwer_weight * sum_b R_b + ctc_weight * sum_b nll_b``,  ``R_b = sum_n P_n d(h_n, targets_b)``,  ``P = softmax_n(loglik_n)``.

    ``decoder``: a ``BeamDecoder`` (its ``decode_nbest_ids`` makes the list; ``nbest <= decoder.beam_width``).  Called like ``CTCLoss``
    with ``(log_probs [T,B,C], targets, input_lengths, target_lengths)``; the value is a sum over the batch (``reduction='sum'``: the
    training loop's ``/ batch_size`` applies unchanged).  Inside one autograd Function, on ``log_probs.detach()``:
    ``decoder.decode_nbest_ids`` -> ``hip_model.ctc_nbest`` (fp64, no round trip through fp32) -> ``hip_model.nbest_mbr`` with the
    targets as reference and uniform weights (for ``ref_dist`` alone) -> ``hip_model.nbest_risk`` -> ``hip_model.ctc_nbest_grad``; the
    saved gradient is scaled by the upstream scalar in ``backward``.  The list is a constant of the step: no gradient flows through the
    search.  An utterance the chain flags (a search status, no hypothesis that is a CTC path, a target id outside the classes) adds 0
    to the risk term and zero rows to its gradient; the CTC term is ``CTCLoss``'s for every utterance.  Where ``ctc_nbest_fits`` or
    ``ctc_nbest_grad_fits`` refuses the shape (or with ``per_rank=True``) the log-likelihoods and the gradient come from one
    ``hip_model.ctc_loss`` call per rank with the same coefficients.  ``ctc_weight`` 0.01 is the paper's interpolation weight: a default,
    not a claim about this model.  ``last`` keeps the step's device tensors (list, loglik, ref_dist, post, risk, coef, flag, nll).

    Out of scope: adding the annotated sequence to the list when the search did not find it; sampled lists; length-normalised
    posteriors."""

    def __init__(self, decoder, nbest, ctc_weight=0.01, mwer_weight=1.0, blank=0, per_rank=False):
        super(MWERLoss, self).__init__()
        if not 2 <= int(nbest) <= min(256, decoder.beam_width):
            raise ValueError("MWERLoss: nbest must be in [2, min(256, beam_width = %d)]" % decoder.beam_width)
        self.decoder, self.nbest, self.ctc_weight, self.mwer_weight, self.blank = decoder, int(nbest), float(ctc_weight), float(mwer_weight), blank
        self.per_rank, self.last = per_rank, None

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        dev = log_probs.device
        il = torch.as_tensor(input_lengths, dtype=torch.int64).to(dev)
        tl = torch.as_tensor(target_lengths, dtype=torch.int64).to(dev)
        tg = _padded_targets(targets, target_lengths).to(dev)
        return _MWERLossFn.apply(log_probs, tg, il, tl, self)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's update (no amsgrad) with the arithmetic in mdd_adam_step: g += weight_decay * p; biased first and
    second moments; bias-corrected step (the betas reach the library as the Python doubles they are: 1 - beta and the bias corrections are
    rounded to fp32 once, as torch rounds them, so exp_avg_sq stays fp32-close to torch's).  State keys ('step', 'exp_avg', 'exp_avg_sq') follow torch's, so a state_dict saved
    by either loads into the other (save_package keeps 'optim_dict', model_ctc.py:262)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super(Adam, self).__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        L = _lib.lib()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
            steps = {int(self.state[p]["step"]) for p in ps}
            for step in steps:                                       # parameters added later may be at a different step
                grp = [p for p in ps if int(self.state[p]["step"]) == step]
                for p in grp:
                    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()):
                        raise RuntimeError("mdd Adam: parameters and gradients must be contiguous float32 CUDA tensors")
                n = len(grp)
                arr = _lib.ptr_array
                numel = (C.c_int64 * n)(*[p.numel() for p in grp])
                with torch.cuda.device(grp[0].device):
                    _lib.check(L.mdd_adam_step(arr(grp), arr([p.grad for p in grp]), arr([self.state[p]["exp_avg"] for p in grp]),
                                               arr([self.state[p]["exp_avg_sq"] for p in grp]), numel, n, step, C.c_float(group["lr"]),
                                               C.c_double(group["betas"][0]), C.c_double(group["betas"][1]), C.c_float(group["eps"]),
                                               C.c_float(group["weight_decay"]), _lib.current_stream_ptr()))
        return loss
