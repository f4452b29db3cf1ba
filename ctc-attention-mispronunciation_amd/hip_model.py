"""Thin object over the C ABI for callers that hold a state_dict of numpy arrays / tensors and want
``forward`` without constructing torch modules (bench.py, tests, the sharded driver).  The
reference-shaped drop-in class is ``models.model_ctc.CTC_Model``, which drives a ``HipModel`` of its own configuration."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib


class HipModel(object):
    """The one owner of a decode handle (mdd_model): made of a synth.Geometry and a state_dict, or of an MddConfig alone (from_config)."""

    def __init__(self, geom, state_dict, device=0, taps=False, precision=None):
        cfg = _lib.MddConfig(feat=geom.feat, hidden=geom.hidden, layers=geom.layers, num_class=geom.num_class,
                             channels=geom.channels, emb_rows=geom.emb_rows, emb_dim=geom.emb_dim, bn_eps=1e-5)
        # a CTC-only geometry (synth.Geometry(ctc_only=True): the reference's cnn-rnn-ctc model) gets the handle without a text side
        self._open(geom, cfg, getattr(geom, "ctc_only", False), device, precision)
        self.load_state_dict(state_dict)
        self.enable_taps(taps)

    @classmethod
    def from_config(cls, cfg, ctc_only, device, precision=None):
        """A handle of ``cfg`` (an MddConfig) on cuda:``device`` with no weights loaded: ``load_state_dict`` before the first forward."""
        self = cls.__new__(cls)
        self._open(None, cfg, ctc_only, device, precision)
        return self

    def _open(self, geom, cfg, ctc_only, device, precision):
        _lib.require_gpu()
        self.geom, self.feat, self.num_class, self._taps = geom, cfg.feat, cfg.num_class, False
        self.device = torch.device("cuda", device)
        self.handle = _lib.new_handle(_lib.lib().mdd_create_ctc if ctc_only else _lib.lib().mdd_create, cfg, device)
        if precision is not None:      # 'f32x6' (fp32-grade on the bf16 matrix cores: the default), 'f32' (exact fp32 MFMA) or 'bf16x3' (flagged variant)
            _lib.check(_lib.lib().mdd_set_precision(self.handle, _lib.PRECISIONS[precision]))

    @property
    def precision(self):
        return {mode: name for name, mode in _lib.PRECISIONS.items()}[_lib.lib().mdd_get_precision(self.handle)]

    def load_state_dict(self, state_dict):
        """Every float entry (numpy array or tensor of any float dtype, converted to fp32 on the host), then mdd_finalize_weights."""
        L = _lib.lib()
        for key, val in state_dict.items():
            if torch.is_tensor(val):     # (bf16 has no numpy form)
                val = val.detach().to("cpu", torch.float32 if val.is_floating_point() else val.dtype).numpy()
            a = np.asarray(val)
            if a.dtype.kind != "f":
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
            _lib.check(L.mdd_load_weight(self.handle, key.encode(), _lib.ptr(a), shape, a.ndim))
        _lib.check(L.mdd_finalize_weights(self.handle))

    def enable_taps(self, on=True):
        """Keep the stage outputs of a forward for ``tap``.  Called only on a change of state: mdd_enable_taps drops the captured graphs."""
        if bool(on) != self._taps:
            _lib.check(_lib.lib().mdd_enable_taps(self.handle, int(bool(on))))
            self._taps = bool(on)

    def _run(self, entry, like, B, T, out, sync_errors, args):
        """Allocate logp [T/2,B,C] unless given, enqueue ``entry(handle, *args, out, stream)`` and, on request, wait and raise device-side errors."""
        if out is None:
            out = torch.empty((T // 2, B, self.num_class), dtype=torch.float32, device=like.device)
        _lib.check(entry(self.handle, *args, _lib.ptr(out), _lib.current_stream_ptr()))
        if sync_errors:
            _lib.raise_device_error(_lib.lib().mdd_sync, self.handle)
        return out

    @staticmethod
    def _ids(x1):
        """(device pointer, L) of the canonical ids; x1 = None (a CTC-only handle ignores them) passes NULL, 0."""
        if x1 is None:
            return None, 0
        assert x1.is_cuda and x1.dtype == torch.int64 and x1.is_contiguous()
        return _lib.ptr(x1), x1.shape[1]

    def forward(self, x, x1=None, out=None, sync_errors=False):
        """x [B,T,F] f32 cuda, x1 [B,L] i64 cuda (None for a CTC-only model) -> logp [T/2,B,C] (enqueued on the current stream)."""
        assert x.is_cuda and x.dtype == torch.float32
        x, x1 = x.contiguous(), (None if x1 is None else x1.contiguous())
        B, T, _ = x.shape
        return self._run(_lib.lib().mdd_forward, x, B, T, out, sync_errors, (_lib.ptr(x), B, T) + self._ids(x1))

    def forward_fused(self, x, x1, frames, canon=None, out=None, sync_errors=False):
        """Several reference batches of different padded lengths in one launch sequence (mdd_forward_fused): x [B,T,F] with every
        batch zero-padded to the common T, x1 [B,L]; frames [B] int32 = T_g/2 and canon [B] int32 = L_g of each row's own batch.
        Rows t < frames[b] of the result equal forward() on that batch alone, bit for bit.  A CTC-only model takes x1 = canon = None."""
        assert x.is_cuda and x.dtype == torch.float32 and frames.is_cuda and frames.dtype == torch.int32
        assert canon is None or (canon.is_cuda and canon.dtype == torch.int32)
        x, frames = x.contiguous(), frames.contiguous()
        x1, canon = (None if x1 is None else x1.contiguous()), (None if canon is None else canon.contiguous())
        B, T, _ = x.shape
        return self._run(_lib.lib().mdd_forward_fused, x, B, T, out, sync_errors,
                         (_lib.ptr(x), B, T) + self._ids(x1) + (_lib.ptr(frames), _lib.ptr(canon)))

    def forward_candidates(self, x, x1, frames=None, canon=None, out=None, sync_errors=False):
        """K canonical candidates per utterance on one acoustic pass (mdd_forward_candidates): x [B,T,F] f32 cuda, x1 [K,B,L] i64 cuda, candidate
        set k being the B utterances with the canonicals x1[k]; frames [B] int32 = T_g/2 as in forward_fused (None: T/2), canon [K*B] (or [K,B])
        int32 = the padded canonical length of each set (None: L).  Returns logp [K,T/2,B,C]: entry k is what forward_fused gives rows k*B .. of
        x repeated K times, bit for bit, and what forward(x, x1[k][:, :L_k]) gives wherever B and K*B rows run the same kernels
        (include/mdd_hip.h)."""
        assert x.is_cuda and x.dtype == torch.float32
        assert x1.is_cuda and x1.dtype == torch.int64 and x1.dim() == 3 and x1.shape[1] == x.shape[0]
        assert frames is None or (frames.is_cuda and frames.dtype == torch.int32 and frames.numel() == x.shape[0])
        assert canon is None or (canon.is_cuda and canon.dtype == torch.int32 and canon.numel() == x1.shape[0] * x1.shape[1])
        x, x1 = x.contiguous(), x1.contiguous()
        frames, canon = (None if frames is None else frames.contiguous()), (None if canon is None else canon.contiguous())
        B, T, _ = x.shape
        K, _, L = x1.shape
        if out is None:
            out = torch.empty((K, T // 2, B, self.num_class), dtype=torch.float32, device=x.device)
        p = _lib.ptr
        return self._run(_lib.lib().mdd_forward_candidates, x, B, T, out, sync_errors, (p(x), B, T, p(x1), K, L, p(frames), p(canon)))

    def forward_raw(self, raw, x1=None, out=None, sync_errors=False):
        """raw [B,T_raw,F/3] f32 cuda (unstacked frames), x1 [B,L] i64 cuda -> logp, exactly as
        forward(stack_features(raw), x1): the stack/skip of data_loader.py:138-142 is applied on the fly."""
        assert raw.is_cuda and raw.dtype == torch.float32
        raw, x1 = raw.contiguous(), (None if x1 is None else x1.contiguous())
        B, T_raw, D = raw.shape
        assert 3 * D == self.feat
        return self._run(_lib.lib().mdd_forward_raw, raw, B, _lib.lib().mdd_stack_len(T_raw, 2, 2), out, sync_errors,
                         (_lib.ptr(raw), B, T_raw) + self._ids(x1))

    def profile(self, x, x1=None):
        """Per-stage (name, ms, launches, flops) of one forward replayed stage by stage between HIP events."""
        B, T, _ = x.shape
        x1p, L = self._ids(x1)
        out = torch.empty((T // 2, B, self.num_class), dtype=torch.float32, device=x.device)
        n = _lib.lib().mdd_forward_num_stages(self.handle)
        names = C.create_string_buffer(64 * n)
        ms, launches, flops = (C.c_float * n)(), (C.c_int32 * n)(), (C.c_double * n)()
        _lib.check(_lib.lib().mdd_forward_profile(self.handle, _lib.ptr(x), B, T, x1p, L, _lib.ptr(out), _lib.current_stream_ptr(),
                                                  names, 64 * n, ms, launches, flops, n))
        return list(zip(names.value.decode().split(","), list(ms), list(launches), list(flops)))

    def tap(self, name):
        """Stage output of the last forward as a torch tensor (copy): conv1, rnn<i>, text, key."""
        n = C.c_int64(0)
        if not _lib.lib().mdd_tap(self.handle, name.encode(), C.byref(n)):
            raise KeyError(name)
        out = torch.empty(n.value, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().mdd_tap_copy(self.handle, name.encode(), _lib.ptr(out), n.value, _lib.current_stream_ptr()))
        return out

    def close(self):
        if self.handle:
            _lib.lib().mdd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class _CtcCall(object):
    """What the six CTC lattice functions share: ``logp`` contiguous fp32 [T,B,C] on its device, conversion of the other arrays to that
    device, and one call of an entry that ends ``..., workspace_dev, workspace_bytes, stream`` (``ctc_nbest``'s: ``..., stream``)."""

    def __init__(self, logp):
        assert logp.is_cuda and logp.dtype == torch.float32
        self.logp = logp.contiguous()
        self.T, self.B, self.C = self.logp.shape
        self.dev = self.logp.device
        self.ws = None

    def to(self, x, dtype):
        return torch.as_tensor(x).to(self.dev, dtype).contiguous()

    def empty(self, shape, dtype, want=True):
        return torch.empty(shape, dtype=dtype, device=self.dev) if want else None

    def workspace(self, bytes_fn, *shape):
        """The call's scratch from torch's caching allocator (stream-ordered, no hipMalloc per call), sized by ``bytes_fn(T, B, C, *shape)``."""
        nws = bytes_fn(self.T, self.B, self.C, *shape)
        self.ws = torch.empty((max(nws, 16) + 7) // 8, dtype=torch.float64, device=self.dev)

    def ptr(self, t, rows=1):
        """Device address of ``t`` (None: NULL); an empty [B, 0] array (``rows`` = 0) passes the workspace's address in its place."""
        return _lib.ptr(t if rows or t is None else self.ws)

    def __call__(self, entry, *args):
        """``entry(logp, T, B, C, *args, workspace_dev, workspace_bytes, stream)``; an entry without a workspace (no ``workspace`` call
        before this one: mdd_ctc_nbest) ends ``..., stream``."""
        tail = () if self.ws is None else (self.ptr(self.ws), self.ws.numel() * 8)
        with torch.cuda.device(self.dev):
            _lib.check(entry(self.ptr(self.logp), self.T, self.B, self.C, *args, *tail, _lib.current_stream_ptr()))


def ctc_loss(logp, targets, in_len, tgt_len, blank=0, want_grad=True):
    """nn.CTCLoss(reduction='sum') pieces on the GPU: returns (nll [B], grad [T,B,C] or None)."""
    c = _CtcCall(logp)
    tg, il, tl = c.to(targets, torch.int64), c.to(in_len, torch.int64), c.to(tgt_len, torch.int64)
    nll = c.empty((c.B,), torch.float32)
    grad = torch.empty_like(c.logp) if want_grad else None
    c.workspace(_lib.lib().mdd_ctc_workspace_bytes, tg.shape[1], 1 if want_grad else 0)
    c(_lib.lib().mdd_ctc_loss, c.ptr(tg), tg.shape[1], c.ptr(il), c.ptr(tl), blank, c.ptr(nll), c.ptr(grad))
    return nll, grad


def ctc_nbest_fits(T, C, max_len):
    """Whether ``ctc_nbest`` takes posteriors of T frames and C classes with hypotheses of up to ``max_len`` ids (mdd_ctc_nbest_fits: at
    most 255 ids, and the [T, C] fp32 block of an utterance within the kernel's LDS bound).  Host only."""
    return bool(_lib.lib().mdd_ctc_nbest_fits(int(T), int(C), int(max_len)))


def ctc_nbest(logp, lens, ids, nids, blank=0, max_len=None):
    """Exact CTC log-likelihood of every hypothesis of an N-best list in one launch (mdd_ctc_nbest).

    logp [T,B,C] fp32 CUDA, lens [B]; ids [N,B,pitch] / nids [N,B] as ``BeamDecoder.decode_nbest_ids`` returns them (int32 CUDA tensors
    pass through with no copy).  ``max_len`` bounds nids (default: the ids' row length, so the call needs no sync); the shape must be one
    ``ctc_nbest_fits`` accepts.  Returns ``loglik [N,B]`` float64 on the device: ``(-loglik).float()`` has the bits of ``ctc_loss``'s nll
    for ``ids[n]``, so -inf where a hypothesis is no CTC path of the frames and NaN where one of its ids is outside the classes.  Nothing
    synchronises."""
    c = _CtcCall(logp)
    lens, ids, nids = c.to(lens, torch.int32), c.to(ids, torch.int32), c.to(nids, torch.int32)
    if ids.dim() != 3 or ids.shape[1] != c.B or lens.shape != (c.B,) or nids.shape != ids.shape[:2]:
        raise ValueError("ctc_nbest: lens [B], ids [N, B, pitch], nids [N, B]")
    N, _, pitch = ids.shape
    Lmax = pitch if max_len is None else int(max_len)
    loglik = c.empty((N, c.B), torch.float64)
    # (rows of no ids at all: nothing is read through ids_dev, which must still be an address)
    c(_lib.lib().mdd_ctc_nbest, c.ptr(lens), c.ptr(ids if pitch else nids), pitch, c.ptr(nids), N, Lmax, blank, c.ptr(loglik))
    return loglik


def ctc_nbest_grad_fits(T, C, max_len):
    """Whether ``ctc_nbest_grad`` takes posteriors of T frames and C classes with hypotheses of up to ``max_len`` ids
    (mdd_ctc_nbest_grad_fits: at most 255 ids, and the [T, C] block, an accumulator of its size and the lattice's arrays within a
    workgroup's LDS; every shape it accepts ``ctc_nbest_fits`` accepts).  Host only."""
    return bool(_lib.lib().mdd_ctc_nbest_grad_fits(int(T), int(C), int(max_len)))


def ctc_nbest_grad(logp, lens, ids, nids, coef, blank=0, max_len=None, want_loglik=False):
    """``grad[t,b,c] = sum_n coef[n,b] g_n[t,b,c]`` in one call (mdd_ctc_nbest_grad), g_n the tensor ``ctc_loss`` deposits on the log-probs
    for hypothesis n as target: the gradient of the MWER objective with ``nbest_risk``'s coefficients.

    logp, lens, ids, nids, max_len as ``ctc_nbest`` takes them; coef [N,B] float64.  A rank with ``coef == 0`` is not scanned.  The shape
    must be one ``ctc_nbest_grad_fits`` accepts.  Returns device tensors ``(grad [T,B,C] f32, flag [B] i32, loglik [N,B] f64 | None)``:
    flag 1 where a rank with a non-zero coef is no CTC path of the frames, 2 where one has an id outside the classes or a coef is not
    finite -- such an utterance has all-zero rows; loglik has ``ctc_nbest``'s bits on scanned ranks and NaN on skipped ones.  Nothing
    synchronises."""
    c = _CtcCall(logp)
    lens, ids, nids, coef = c.to(lens, torch.int32), c.to(ids, torch.int32), c.to(nids, torch.int32), c.to(coef, torch.float64)
    if ids.dim() != 3 or ids.shape[1] != c.B or lens.shape != (c.B,) or nids.shape != ids.shape[:2] or coef.shape != ids.shape[:2]:
        raise ValueError("ctc_nbest_grad: lens [B], ids [N, B, pitch], nids [N, B], coef [N, B]")
    N, _, pitch = ids.shape
    Lmax = pitch if max_len is None else int(max_len)
    grad, flag = torch.empty_like(c.logp), c.empty((c.B,), torch.int32)
    loglik = c.empty((N, c.B), torch.float64, want_loglik)
    c.workspace(_lib.lib().mdd_ctc_nbest_grad_workspace_bytes, N, Lmax)
    c(_lib.lib().mdd_ctc_nbest_grad, c.ptr(lens), c.ptr(ids if pitch else nids), pitch, c.ptr(nids), N, Lmax, blank, c.ptr(coef), c.ptr(loglik),
      c.ptr(grad), c.ptr(flag))
    return grad, flag, loglik


def nbest_risk(loglik, cost, status=None):
    """Posteriors, risk and MWER coefficients of an N-best list (mdd_nbest_risk): loglik [N,B] float64 (``ctc_nbest``'s), cost [N,B] int32
    (``nbest_mbr``'s ref_dist), status [B] or None.  Returns device tensors ``(post [N,B] f64, risk [B] f64, coef [N,B] f64, flag [B]
    i32)``: post the softmax over the ranks with a finite loglik, risk = sum post cost, coef = post (risk - cost) = d risk / d nll.
    flag 1 (status non-zero, or no finite rank) or 2 (a negative cost) gives post and coef 0 and risk NaN.  Nothing synchronises."""
    loglik = torch.as_tensor(loglik)
    if not loglik.is_cuda:
        _lib.require_gpu()
    loglik = _lib.to_gpu(loglik, torch.float64)
    dev = loglik.device
    cost = torch.as_tensor(cost).to(dev, torch.int32).contiguous()
    status = None if status is None else torch.as_tensor(status).to(dev, torch.int32).contiguous()
    if loglik.dim() != 2 or cost.shape != loglik.shape or (status is not None and status.shape != loglik.shape[1:]):
        raise ValueError("nbest_risk: loglik [N, B], cost [N, B], status [B]")
    N, B = loglik.shape
    post, coef = torch.empty_like(loglik), torch.empty_like(loglik)
    risk, flag = torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mdd_nbest_risk(p(loglik), p(cost), p(status), N, B, p(post), p(risk), p(coef), p(flag), _lib.current_stream_ptr()))
    return post, risk, coef, flag


AlignResult =collections.namedtuple("AlignResult", "score status path seg seg_logp")
ALIGN_OK, ALIGN_INFEASIBLE, ALIGN_BAD_TARGET = 0, 1, 2      # include/mdd_hip.h: mdd_align_status


def ctc_align(logp, lens, ids, nids, blank=0, max_len=None, want_path=True, want_segments=True):
    """CTC forced alignment on the GPU (mdd_ctc_align): the best path of ``ids`` through ``logp``.

    logp [T,B,C] fp32 CUDA, lens [B], ids [B,stride] / nids [B] as ``decode_ids`` returns them (int32 CUDA tensors pass through with
    no copy).  ``max_len`` bounds nids (default: ids.shape[1], so the call needs no sync).  Returns
    ``AlignResult(score [B] f32, status [B] i32, path [B,T] i32 | None, seg [B,stride,2] i32 | None, seg_logp [B,stride] f32 | None)``:
    path[b,t] is the position of the label frame t emits or -1, seg[b,i] the first and one-past-last frame of label i, seg_logp[b,i]
    the sum of its frames' log-posteriors.  Nothing synchronises."""
    c = _CtcCall(logp)
    B = c.B
    lens, ids, nids = c.to(lens, torch.int32), c.to(ids, torch.int32), c.to(nids, torch.int32)
    if ids.dim() != 2 or ids.shape[0] != B or lens.shape != (B,) or nids.shape != (B,):
        raise ValueError("ctc_align: lens [B], ids [B, stride], nids [B]")
    stride = ids.shape[1]
    Lmax = stride if max_len is None else int(max_len)
    score, status = c.empty((B,), torch.float32), c.empty((B,), torch.int32)
    path = c.empty((B, c.T), torch.int32, want_path)
    seg, seg_logp = c.empty((B, stride, 2), torch.int32, want_segments), c.empty((B, stride), torch.float32, want_segments)
    c.workspace(_lib.lib().mdd_ctc_align_workspace_bytes, max(Lmax, 0))
    c(_lib.lib().mdd_ctc_align, c.ptr(lens), c.ptr(ids, stride), stride, c.ptr(nids), Lmax, blank, c.ptr(score), c.ptr(status), c.ptr(path),
      c.ptr(seg), c.ptr(seg_logp))
    return AlignResult(score, status, path, seg, seg_logp)


VariantResult = collections.namedtuple("VariantResult", "base sub ins status")


def ctc_variants(logp, lens, ids, nids, blank=0, max_len=None, want_ins=True):
    """CTC log-likelihood of every sequence one edit away from ``ids`` (mdd_ctc_variants), from two lattices per utterance.

    logp [T,B,C] fp32 CUDA, lens [B], ids [B,stride] / nids [B] as ``ctc_align`` takes them (int32 CUDA tensors pass through with no
    copy); ``max_len`` bounds nids (default: ids.shape[1], so the call needs no sync).  Returns
    ``VariantResult(base [B] f64, sub [B,stride,C] f64, ins [B,stride+1,C] f64 | None, status [B] i32)``, absolute log-likelihoods:
    sub[b,i,k] with ids[i] replaced by k (k == blank: ids[i] deleted; k == ids[i]: base), ins[b,g,k] with k inserted before position g
    (k == blank: base); rows past nids[b] are -inf up to ``max_len`` and not written beyond it.  Nothing synchronises."""
    c = _CtcCall(logp)
    B = c.B
    lens, ids, nids = c.to(lens, torch.int32), c.to(ids, torch.int32), c.to(nids, torch.int32)
    if ids.dim() != 2 or ids.shape[0] != B or lens.shape != (B,) or nids.shape != (B,):
        raise ValueError("ctc_variants: lens [B], ids [B, stride], nids [B]")
    stride = ids.shape[1]
    Lmax = stride if max_len is None else int(max_len)
    base, status = c.empty((B,), torch.float64), c.empty((B,), torch.int32)
    sub = c.empty((B, stride, c.C), torch.float64)
    ins = c.empty((B, stride + 1, c.C), torch.float64, want_ins)
    c.workspace(_lib.lib().mdd_ctc_variants_workspace_bytes, max(Lmax, 0))
    c(_lib.lib().mdd_ctc_variants, c.ptr(lens), c.ptr(ids, stride), stride, c.ptr(nids), Lmax, blank, c.ptr(base), c.ptr(sub, stride), c.ptr(ins),
      c.ptr(status))
    return VariantResult(base, sub, ins, status)


ConfnetResult = collections.namedtuple("ConfnetResult", "total post status")


def ctc_confnet_max_slots(num_class):
    """The largest ``max_slots`` ``ctc_confnet`` accepts for ``num_class`` classes (mdd_ctc_confnet_max_slots: the kernel's LDS rows)."""
    return int(_lib.lib().mdd_ctc_confnet_max_slots(int(num_class)))


def ctc_confnet(logp, lens, w, nslots, blank=0, max_slots=None, want_post=True):
    """CTC over an error network (mdd_ctc_confnet): every slot of an utterance offers C weighted entries, a reading picks one per slot.

    logp [T,B,C] fp32 CUDA, lens [B] as ``ctc_variants`` takes them; w [B,stride,C] fp32 log-weights (entry k != blank: the slot emits
    k; k == blank: it emits nothing; -inf: no such arc; rows need not be normalised), nslots [B] the slots in use; ``max_slots`` bounds
    nslots (default: w.shape[1], so the call needs no sync).  Returns ``ConfnetResult(total [B] f64, post [B,stride,C] f64 | None,
    status [B] i32)``, absolute log values: total over all readings (weights + CTC log-likelihood of the emitted labels), post[b,j,k]
    over the readings that pick entry k in slot j -- exp(post - total) is the posterior; rows past nslots[b] are -inf up to
    ``max_slots`` and not written beyond it.  Nothing synchronises."""
    c = _CtcCall(logp)
    B = c.B
    lens, w, nslots = c.to(lens, torch.int32), c.to(w, torch.float32), c.to(nslots, torch.int32)
    if w.dim() != 3 or w.shape[0] != B or w.shape[2] != c.C or lens.shape != (B,) or nslots.shape != (B,):
        raise ValueError("ctc_confnet: lens [B], w [B, stride, C], nslots [B]")
    stride = w.shape[1]
    Jmax = stride if max_slots is None else int(max_slots)
    total, status = c.empty((B,), torch.float64), c.empty((B,), torch.int32)
    post = c.empty((B, stride, c.C), torch.float64, want_post)
    c.workspace(_lib.lib().mdd_ctc_confnet_workspace_bytes, max(Jmax, 0), 1 if want_post else 0)
    c(_lib.lib().mdd_ctc_confnet, c.ptr(lens), c.ptr(w, stride), stride, c.ptr(nslots), Jmax, blank, c.ptr(total), c.ptr(post, stride), c.ptr(status))
    return ConfnetResult(total, post, status)


ConfnetBestResult = collections.namedtuple("ConfnetBestResult", "score reading status path seg")


def ctc_confnet_best(logp, lens, w, nslots, blank=0, max_slots=None, want_path=True, want_segments=True):
    """The best reading of an error network with its alignment (mdd_ctc_confnet_best): the max-product sweep over ``ctc_confnet``'s network.

    Arguments as ``ctc_confnet`` takes them.  Returns ``ConfnetBestResult(score [B] f64, reading [B,stride] i32, status [B] i32, path
    [B,T] i32 | None, seg [B,stride,2] i32 | None)``: score is the largest sum of a reading's weights and one CTC path's log-posteriors
    (the best pair of reading and alignment, not the reading of the largest summed likelihood); reading[b,j] the entry slot j takes
    (``blank``: it emits nothing); path[b,t] the slot whose label frame t emits or -1; seg[b,j] the first and one-past-last frame of slot
    j's label, -1, -1 where it emits nothing.  Rows past nslots[b] are -1 up to ``max_slots`` and not written beyond it.  Nothing
    synchronises."""
    c = _CtcCall(logp)
    B = c.B
    lens, w, nslots = c.to(lens, torch.int32), c.to(w, torch.float32), c.to(nslots, torch.int32)
    if w.dim() != 3 or w.shape[0] != B or w.shape[2] != c.C or lens.shape != (B,) or nslots.shape != (B,):
        raise ValueError("ctc_confnet_best: lens [B], w [B, stride, C], nslots [B]")
    stride = w.shape[1]
    Jmax = stride if max_slots is None else int(max_slots)
    score, status = c.empty((B,), torch.float64), c.empty((B,), torch.int32)
    reading = c.empty((B, stride), torch.int32)
    path = c.empty((B, c.T), torch.int32, want_path)
    seg = c.empty((B, stride, 2), torch.int32, want_segments)
    c.workspace(_lib.lib().mdd_ctc_confnet_best_workspace_bytes, max(Jmax, 0))
    c(_lib.lib().mdd_ctc_confnet_best, c.ptr(lens), c.ptr(w, stride), stride, c.ptr(nslots), Jmax, blank, c.ptr(score), c.ptr(reading, stride),
      c.ptr(status), c.ptr(path), c.ptr(seg, stride))
    return ConfnetBestResult(score, reading, status, path, seg)


MBR_MAX_LEN = 1024          # include/mdd_hip.h: mdd_nbest_mbr's bound on max_len (16 words of 64 pattern positions)


def nbest_mbr(ids, nids, status, weights, num_class, max_len=None, ref=None, ref_len=None, want_dist=False):
    """Minimum-Bayes-risk decode of an N-best list on the GPU (mdd_nbest_mbr): every pairwise edit distance inside each utterance's list,
    each hypothesis' expected distance under the list's own weights, and the hypothesis that minimises it.

    ids [N,B,pitch] / nids [N,B] int32 as ``BeamDecoder.decode_nbest_ids`` returns them (int32 CUDA tensors pass through with no copy),
    status [B] or None (non-zero: skip the utterance), weights [N,B] float64, finite and >= 0 (``nbest_posteriors``' shares; they need
    not sum to 1).  ``max_len`` bounds nids (default: the ids' row length clipped to the limit of 1024, so the call needs no sync); a
    bound of at most 64 runs the kernel's one-word form.  ``ref`` [B,ref_pitch] / ``ref_len`` [B]: a reference sequence per utterance,
    both or neither.  Returns device tensors ``(best [B] i32, risk [N,B] f64, flag [B] i32, dist [B,N,N] i32 | None, ref_dist [N,B] i32 |
    None, ref_risk [B] f64 | None)``: risk[n,b] = sum_m weights[m,b] d(h_n, h_m); best[b] the lowest n with a weight above 0 and the
    least risk; ref_dist[n,b] = d(h_n, ref_b) and ref_risk[b] their weighted sum.  flag[b] = 1 (skipped: status, or no weight above 0)
    or 2 (a length outside [0, max_len] or an id outside [0, num_class)) gives best -1, NaN risks and -1 distances.  Nothing
    synchronises."""
    ids = torch.as_tensor(ids)
    if not ids.is_cuda:
        _lib.require_gpu()
    ids = _lib.to_gpu(ids, torch.int32)
    dev = ids.device

    def to(x, dtype):
        return None if x is None else torch.as_tensor(x).to(dev, dtype).contiguous()

    nids, status, weights, ref, ref_len = to(nids, torch.int32), to(status, torch.int32), to(weights, torch.float64), to(ref, torch.int32), to(ref_len, torch.int32)
    if ids.dim() != 3 or nids.shape != ids.shape[:2] or weights.shape != ids.shape[:2] or (status is not None and status.shape != ids.shape[1:2]):
        raise ValueError("nbest_mbr: ids [N, B, pitch], nids [N, B], status [B], weights [N, B]")
    N, B, pitch = ids.shape
    if (ref is None) != (ref_len is None) or (ref is not None and (ref.dim() != 2 or ref.shape[0] != B or ref_len.shape != (B,))):
        raise ValueError("nbest_mbr: ref [B, ref_pitch] and ref_len [B], both or neither")
    L = min(pitch, MBR_MAX_LEN) if max_len is None else int(max_len)
    has_ref = ref is not None
    ref_pitch = ref.shape[1] if has_ref else 0
    if has_ref and ref_pitch == 0:           # an empty [B, 0] reference: every length must be 0; one never-read column stands in
        ref, ref_pitch = torch.zeros((B, 1), dtype=torch.int32, device=dev), 1

    def empty(shape, dtype, want=True):
        return torch.empty(shape, dtype=dtype, device=dev) if want else None

    best, risk, flag = empty((B,), torch.int32), empty((N, B), torch.float64), empty((B,), torch.int32)
    dist = empty((B, N, N), torch.int32, want_dist)
    ref_dist, ref_risk = empty((N, B), torch.int32, has_ref), empty((B,), torch.float64, has_ref)
    L_ = _lib.lib()
    nws = L_.mdd_nbest_mbr_workspace_bytes(N, B, int(num_class), L)
    ws = torch.empty((max(nws, 16) + 7) // 8, dtype=torch.float64, device=dev)      # torch's caching allocator: no hipMalloc per call
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(L_.mdd_nbest_mbr(p(ids), pitch, p(nids), p(status), p(weights), N, B, int(num_class), L, p(ref), p(ref_len), ref_pitch,
                                    p(best), p(risk), p(dist), p(ref_dist), p(ref_risk), p(flag), p(ws), ws.numel() * 8,
                                    _lib.current_stream_ptr()))
    return best, risk, flag, dist, ref_dist, ref_risk
