"""CTC loss cases at the shapes where ``mdd_ctc_loss`` (csrc/ctc.hip) changes its kernel, with a float64 reference, shared by
tests/test_ctc_loss_reference.py (CPU: the table itself, the form rule against the library's workspace size, the conditions on the inputs),
tests/test_ctc_loss_forms.py (GPU: both kernels against the reference) and tools/ctc_loss_margins.py (the measured margins).

The reference (``reference``) is CPU ``torch.nn.functional.ctc_loss`` on a double tensor with ``reduction='none'`` -- the call
tests/test_ctc_variants.py::brute makes for the lattice -- and ``nll.sum().backward()`` for the gradient on the log-probs.  ``aten_fp32`` is
the same call on the fp32 tensor: the same operation at the reference project's own width, the yardstick a kernel's error is held beside.

``expected_form`` restates ctc_wave_form / ctc_labels_per_lane / wave_smem of csrc/ctc.hip and csrc/ctc_host.h: the wave kernel with 1, 2 or
4 labels per lane when Lmax <= 255, C <= 256 and the staged log-probs with the kernel's lists fit 128 KB of LDS, the generic kernel
otherwise.

Rows: row 0 has full lengths, row 1 ragged input and label lengths, row 2 (every case but "ends") no labels at all (tl = 0) beside rows that
have some.  Labels avoid the blank, carry no adjacent repeats but two forced ones (a blank is needed between them), and reach the last class.
"ends" is test_ctc_edge_cases_against_oracle's batch of four rows (a barely feasible row of one label, a row of one frame) with the blank at
class 0 and at class 6.

The clamp case hands the kernels ``il = [T + 7, -2, T]``; both clamp to [0, T], so the reference runs on ``[T, 0, T]`` (``il_ref``).  Row 1
then has no frames and labels to emit (L > 0): the library and the reference both give nll = +inf and a gradient of zero on every frame of the row.
It is the only row of the table whose reference is not finite."""
import collections
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "ctc_loss_margins.json")
WAVE_LDS = 128 * 1024
FORMS = ("wave1", "wave2", "wave4", "generic")
# the project's present bounds for this operation (tests/test_gpu_parity.py::test_ctc_wave_kernel_label_widths_against_oracle)
NLL_RTOL = 1e-6
GRAD_ATOL = {"wave1": 5e-6, "wave2": 5e-6, "wave4": 5e-6, "generic": 2e-6}
MARGIN_FACTOR = 2.0         # other seeds and compiler versions; the kernels are deterministic, so not run-to-run noise
CLASS_SUM = 1e-4            # |sum over classes of a live frame's gradient|, as test_ctc_loss_golden_and_oracle

Spec = collections.namedtuple("Spec", "T C L blank scale kind seed")


def labels_per_lane(Lmax):
    return 1 if Lmax <= 63 else (2 if Lmax <= 127 else 4)


def wave_smem(T, C, NL):
    """Dynamic LDS of ctc_wave_kernel: lpt[T][C] f32 | lab[LC] | cls_off[C + 1] | cls_idx[LC] | gam[8][LC], LC = 64 NL."""
    LC = 64 * NL
    return T * C * 4 + LC * 4 + (C + 1) * 4 + LC * 4 + 8 * LC * 4


def expected_form(T, C, Lmax):
    NL = labels_per_lane(Lmax)
    if Lmax <= 255 and C <= 256 and wave_smem(T, C, NL) <= WAVE_LDS:
        return "wave%d" % NL
    return "generic"


def expected_workspace_bytes(T, B, C, Lmax):
    """mdd_ctc_workspace_bytes with a gradient: the wave form keeps alpha and beta rows of pitch 2 (Lmax + 1), the generic form alpha rows of
    2 Lmax + 1 states."""
    if expected_form(T, C, Lmax) == "generic":
        return 8 * B * T * (2 * Lmax + 1)
    return 16 * B * T * 2 * (Lmax + 1)


def last_wave_T(C, Lmax):
    """The largest T the wave form takes at this C and Lmax (the LDS rule alone)."""
    assert expected_form(1, C, Lmax) != "generic"
    T = 1
    while expected_form(T + 1, C, Lmax) != "generic":
        T += 1
    return T


T101 = last_wave_T(101, 20)     # 317: 404 bytes a frame beside 2,968 bytes of lists

SPECS = collections.OrderedDict([
    # the LDS rule at C = 45, NL = 1: 180 bytes a frame beside 2,744 bytes of lists
    ("lds45_T712", Spec(712, 45, 40, 0, 2.0, "random", 1)),
    ("lds45_T713", Spec(713, 45, 40, 0, 2.0, "random", 2)),
    ("lds101_T%d" % T101, Spec(T101, 101, 20, 0, 2.0, "random", 3)),
    ("lds101_T%d" % (T101 + 1), Spec(T101 + 1, 101, 20, 0, 2.0, "random", 4)),
    ("lane_L127", Spec(147, 45, 127, 0, 2.0, "random", 5)),                  # 2 labels per lane
    ("lane_L128", Spec(148, 45, 128, 0, 2.0, "random", 6)),                  # 4 labels per lane
    ("form_L255", Spec(530, 45, 255, 0, 2.0, "random", 7)),                  # the last label count of the wave form
    ("form_L256", Spec(530, 45, 256, 0, 2.0, "random", 8)),                  # generic, S = 513: one state in the third trip of 256 threads
    ("long_L300", Spec(330, 45, 300, 0, 2.0, "random", 9)),                  # generic, S = 601
    ("wide_C257_blank256", Spec(60, 257, 12, 256, 2.0, "random", 10)),       # generic, class 256 (the blank) in the second trip over classes
    ("wide_C300", Spec(60, 300, 12, 0, 2.0, "random", 11)),                  # generic, 44 classes in the second trip
    ("peaked_x30", Spec(250, 45, 40, 0, 30.0, "random", 12)),                # log-probs to about -210
    ("peaked_x12_blank44", Spec(250, 45, 40, 44, 12.0, "random", 13)),
    ("blank22", Spec(250, 45, 40, 22, 2.0, "random", 14)),                   # the blank neither the first nor the last class
    ("repeats_T81", Spec(81, 45, 40, 0, 2.0, "repeats", 15)),
    ("repeats_T79", Spec(79, 45, 40, 0, 2.0, "repeats", 16)),                # 79 = 2 L - 1: row 0 is feasible by a single path
    ("clamp", Spec(20, 7, 5, 0, 1.0, "clamp", 17)),
    ("ends_blank0", Spec(9, 7, 4, 0, 1.0, "ends", 18)),
    ("ends_blank6", Spec(9, 7, 4, 6, 1.0, "ends", 18)),
])
NAMES = tuple(SPECS)
# neighbouring cases that lie on two sides of a boundary of the form rule
PAIRS = (("lds45_T712", "lds45_T713"), ("lds101_T%d" % T101, "lds101_T%d" % (T101 + 1)), ("lane_L127", "lane_L128"), ("form_L255", "form_L256"))

Case = collections.namedtuple("Case", "name spec lp tg il tl il_ref blank form")


def _log_softmax32(z):
    z = z - z.max(axis=-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=-1, keepdims=True))).astype(np.float32)


def _labels(rs, L, classes, repeats=2):
    """L labels without adjacent repeats, the last class among them, then `repeats` positions made equal to their left neighbour."""
    y = []
    for _ in range(L):
        c = classes[int(rs.integers(len(classes)))]
        while y and c == y[-1]:
            c = classes[int(rs.integers(len(classes)))]
        y.append(c)
    if L > 4:
        y[3] = classes[-1]
        for j in (2, 4):
            if y[j] == y[3]:
                y[j] = classes[0]
    for j in (rs.choice(np.arange(1, L), size=min(repeats, L - 1), replace=False) if L > 1 else []):
        y[j] = y[j - 1]
    return y


def _frames_needed(y):
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case, once: the arrays are shared, so nobody writes into them."""
    s = SPECS[name]
    rs = np.random.Generator(np.random.PCG64(1000 + s.seed))
    T, C, L, blank = s.T, s.C, s.L, s.blank
    classes = [c for c in range(C) if c != blank]
    if s.kind == "ends":
        a, b, c, d, e, f = classes
        rows = [[a, a, a, a], [b, c], [d], [e, f, e, f]]
        il = [9, 5, 1, 9]
    elif s.kind == "repeats":
        k = classes[int(rs.integers(len(classes)))]
        rows = [[k] * L, [k] * 25, []]
        il = [T, 60, T - 9]
    else:
        L1 = L // 2 + int(rs.integers(max(1, L // 4)))
        rows = [_labels(rs, L, classes), _labels(rs, L1, classes), []]
        need = _frames_needed(rows[1])
        il = [T, need + 1 + int(rs.integers(max(1, (T - need) // 2))), T - int(rs.integers(1, max(2, T // 3)))]
        assert _frames_needed(rows[0]) <= T and il[1] <= T
    B = len(rows)
    tg = np.full((B, L), classes[0], dtype=np.int64)      # the padding is a valid label, never read
    for r, y in enumerate(rows):
        tg[r, :len(y)] = y
    tl = np.array([len(y) for y in rows], dtype=np.int64)
    il = np.array(il, dtype=np.int64)
    il_ref = il
    if s.kind == "clamp":
        il, il_ref = np.array([T + 7, -2, T], dtype=np.int64), np.array([T, 0, T], dtype=np.int64)
    lp = _log_softmax32(rs.standard_normal((T, B, C)) * s.scale)
    for a_ in (lp, tg, tl, il, il_ref):
        a_.setflags(write=False)
    return Case(name, s, lp, tg, il, tl, il_ref, blank, expected_form(T, C, L))


def _aten(c, dtype):
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(min(16, torch.get_num_threads()))
    x = torch.from_numpy(np.array(c.lp)).to(dtype).requires_grad_(True)
    nll = F.ctc_loss(x, torch.from_numpy(np.array(c.tg)), torch.from_numpy(np.array(c.il_ref)), torch.from_numpy(np.array(c.tl)),
                     blank=c.blank, reduction="none")
    nll.sum().backward()
    out = nll.detach().numpy().astype(np.float64), x.grad.numpy().astype(np.float64)
    for a_ in out:
        a_.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(nll [B] float64, grad [T, B, C] float64) of the case in float64, once."""
    return _aten(case(name), __import__("torch").float64)


@functools.lru_cache(maxsize=None)
def aten_fp32(name):
    """The same call on the fp32 tensor, its results widened."""
    return _aten(case(name), __import__("torch").float32)


def nll_rel_err(nll, ref):
    """Worst relative error over the rows whose reference is finite; an infinite row must be the same infinity."""
    nll, ref = np.asarray(nll, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert (nll[~fin] == ref[~fin]).all(), (nll, ref)
    return float((np.abs(nll[fin] - ref[fin]) / np.abs(ref[fin])).max(initial=0.0))


def grad_abs_err(grad, ref):
    return float(np.abs(np.asarray(grad, dtype=np.float64) - ref).max())


@functools.lru_cache(maxsize=None)
def aten_err(name):
    """(nll relative error, gradient absolute error) of ATen's fp32 against float64 on this case."""
    (n64, g64), (n32, g32) = reference(name), aten_fp32(name)
    return nll_rel_err(n32, n64), grad_abs_err(g32, g64)


def runs():
    """Every (case, form, forced) the GPU test makes: the routed kernel, and the generic kernel forced on every wave-form case."""
    out = []
    for n in NAMES:
        f = case(n).form
        out.append((n, f, False))
        if f != "generic":
            out.append((n, "generic", True))
    return out


def run_id(name, form, forced):
    return "%s-%s%s" % (name, form, "-forced" if forced else "")


@functools.lru_cache(maxsize=None)
def margins():
    with open(MARGINS) as f:
        return json.load(f)


def bounds(form):
    """(nll rtol, gradient atol) of a kernel form: the larger of the project's present bound and MARGIN_FACTOR x the worst value measured on
    an MI355X over every run of the table in that form (tools/ctc_loss_margins.py -> profiles/ctc_loss_margins.json)."""
    m = [r for r in margins()["runs"].values() if r["form"] == form]
    assert m, form
    return (max(NLL_RTOL, MARGIN_FACTOR * max(r["nll_rel_err"] for r in m)), max(GRAD_ATOL[form], MARGIN_FACTOR * max(r["grad_abs_err"] for r in m)))
