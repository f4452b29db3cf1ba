"""Gate-clear training cases: inputs on which the conv front end's gradients are as well conditioned as every other tensor of the step,
shared by tests/test_conv_train_reference.py (CPU: the conditions that make the bound legitimate, and its teeth) and
tests/test_conv_train.py (GPU: the step against oracle/ref_port.train_step in float64).

Why: behind each of the two conv BatchNorms sits a ReLU, and with N(0,1) inputs a few of the 1e5 .. 1e7 pre-ReLU values y lie within one
fp32 rounding of zero.  One such gate deciding the other way moves a conv gradient by ~1e-3 of its scale, which is why the other training
tests hold conv.* to 3e-3 (DESIGN.md sections 2 and 7) -- a bound under which a lost 128-position tile of the conv1 weight gradient passes at
the large shapes.  The BatchNorm biases are ordinary parameters of the synthetic state dict, and y = gamma . xhat + beta moves as a whole
with beta (the batch statistics do not see it), so clear_gates picks each channel's beta such that zero falls into the middle of the widest
gap between neighbouring values of y.  With every gate decided the same way in fp32 and float64, the distance of a correct fp32 step from
the float64 one on conv.* is rounding-level (ATen's: 6e-7 .. 2e-5), and a wrong index in a conv kernel is not.

The table: name -> Case(geometry kwargs over the reference's, (B, T, L, Lt), runs, seed, window); a run is (mode, conv1-through-im2col
switch).  Unless a case says otherwise the model is SMALL, so that what lies outside the CNN stays cheap.  B * T >= 64 everywhere (well
conditioned batch statistics: tests/geometry_cases.py).  Lt = 1 where T' is 1, 2 or 4: four labels with repeats need up to 7 frames, and
the float64 step of an infeasible row is NaN."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import geometry_cases as gc

P_DROP = 0.2
SMALL = dict(hidden=64, layers=1, num_class=20, emb_rows=19, emb_dim=64)
Case = collections.namedtuple("Case", "geom shape runs seed window")
F32 = (("f32", False),)


def _small(**kw):
    return dict(SMALL, **kw)


CASES = {
    # the shipped widths (W1 = 122, W2 = 61), both conv1 paths and both reference-width modes on the same inputs
    "ref": Case(dict(hidden=256, layers=1), (4, 32, 6, 4), (("f32", False), ("f32x6", False), ("f32", True)), 304, 0.25),
    # 32 * 34 * 61 = 66 368 positions = 519 tiles > 512 workgroups: seven workgroups of conv1_wgrad_direct_kernel walk two tiles
    "gridstride": Case(_small(), (32, 68, 4, 4), F32, 332, 0.25),
    "odd": Case(_small(feat=241), (4, 16, 3, 4), F32, 304, 0.25),            # W1 = 121, W2 = 61: the other right edge of dgrad's classes
    # W1 = 128, W2 = 64: nj = 64, the last width of the direct kernels.  Seed 404, not the table's 300 + B: the draw of seed 304 is ill
    # conditioned in rnns.0's forward recurrence (rounding_response 1.4e-5 against <= 1.5e-6 everywhere else; the GPU step then sits at
    # 6.6e-5 on rnns.0.rnn.weight_ih_l0, in the cell-gate rows and evenly over all w', the same with conv1 through im2col, and ATen fp32
    # at 1.6e-5), which says nothing about an index.  The next seeds (404 .. 704) answer with 7e-7 .. 1.0e-6.
    "last_direct": Case(_small(feat=255), (4, 16, 3, 4), F32, 404, 0.25),
    # W1 = 127: nj = 64 / 63; T' = 11; 66 rows: conv0 backward's 16-row groups, col_stats32's 8- and 32-row steps, mask_rows' tiles end ragged
    "ragged": Case(_small(feat=253), (3, 22, 3, 4), F32, 303, 0.25),
    "first_im2col": Case(_small(feat=257), (4, 16, 3, 4), F32, 304, 0.25),   # W1 = 129 > 128: im2col by width, not by switch
    "one_row_tile2": Case(_small(feat=129), (4, 16, 3, 4), F32, 304, 0.25),  # W1 = 65: nj = 33 / 32, one row in dgrad's second MFMA tile
    "half_tile": Case(_small(feat=120), (5, 16, 3, 4), F32, 305, 0.25),      # W1 = 60: nj = 30, dgrad's second tile empty
    "w3": Case(_small(feat=5), (8, 8, 3, 1), F32, 308, 0.25),                # W1 = 3, W2 = 2: every position on a border
    "w2_feat3": Case(_small(feat=3), (32, 2, 3, 1), F32, 332, 0.25),         # W1 = 2, W2 = 1, T' = 1: the odd input row has one tap row
    "w2_feat4": Case(_small(feat=4), (16, 4, 2, 1), F32, 316, 0.25),         # the other feat with W1 = 2; T' = 2
    # 4 channels: conv1 through im2col + GEMM, the generic col_stats_kernel
    "ch4": Case(dict(feat=39, hidden=20, layers=1, channels=4, num_class=12, emb_rows=11, emb_dim=20), (5, 16, 3, 4), F32, 305, 0.25),
}
RUNS = [(n, mode, im2col) for n in CASES for mode, im2col in CASES[n].runs]


def run_id(name, mode, im2col):
    return "%s-%s%s" % (name, mode, "-im2col" if im2col else "")


def wgrad_tiles(B, T, W2):
    """(tiles, workgroups) of conv1_wgrad_direct_kernel: conv1_wgrad_parts and launch_conv1_wgrad_direct, csrc/train_conv1.hip:238-246 --
    R1 = B * (T / 2) * W2 output positions in tiles of 128, at most 512 workgroups that walk the tiles grid-stride."""
    tiles = (B * (T // 2) * W2 + 127) // 128
    return tiles, min(512, tiles)


def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def pre_relu(sd, x, masks, p, dtype=torch.float64, eps=1e-5):
    """The pre-ReLU tensors (y0 [B, ch, T, W1], y1 [B, ch, T', W2]) of the train-mode CNN, with ref_port.train_step's operations in its
    order: conv, BatchNorm on batch statistics, ReLU, the handed-in dropout mask scaled by 1 / (1 - p).  The masks act after the ReLU, so
    they enter only through conv1's input."""
    def t(k):
        return torch.as_tensor(np.asarray(sd[k])).to(dtype)
    a, ys = torch.as_tensor(x).to(dtype).unsqueeze(1), []
    with torch.no_grad():
        for n, stride in ((0, (1, 2)), (1, (2, 2))):
            z = F.conv2d(a, t("conv.%d.conv.weight" % n), t("conv.%d.conv.bias" % n), stride=stride, padding=(1, 1))
            y = F.batch_norm(z, None, None, t("conv.%d.batch_norm.weight" % n), t("conv.%d.batch_norm.bias" % n), training=True, eps=eps)
            ys.append(y)
            a = F.relu(y)
            if p > 0:
                a = a * (torch.as_tensor(masks[n], dtype=dtype) * (1.0 / (1.0 - p)))
    return ys


def _gap_centres(y, window):
    """Per channel, the middle of the widest gap between neighbouring values of y inside (-window, window); the window's ends count as
    values, so the result lies inside the window and half the gap is a lower bound of the margin after the shift."""
    C = y.shape[1]
    flat = y.transpose(0, 1).reshape(C, -1).numpy()
    out = np.zeros(C, dtype=np.float64)
    for c in range(C):
        v = flat[c]
        v = np.sort(np.concatenate(([-window], v[np.abs(v) < window], [window])))
        i = int(np.argmax(np.diff(v)))
        out[c] = 0.5 * (v[i] + v[i + 1])
    return out


def clear_gates(sd, x, masks, p, window=0.25):
    """A copy of the state dict in which only conv.0.batch_norm.bias and conv.1.batch_norm.bias differ, each entry by at most `window`:
    per channel beta is shifted so that the middle of the widest gap of the float64 pre-ReLU values lands on zero.  Site 0 first, then
    site 1 on the recomputed values (conv1's input depends on site 0's gates).  The biases stay float32, the state dict's type."""
    _threads()
    out = type(sd)((k, np.array(v, copy=True)) for k, v in sd.items())
    for n in (0, 1):
        key = "conv.%d.batch_norm.bias" % n
        shift = _gap_centres(pre_relu(out, x, masks, p)[n], window)
        out[key] = (out[key].astype(np.float64) - shift).astype(np.float32)
    return out


Margin = collections.namedtuple("Margin", "min_abs aten_err flips")


def gate_margin(sd, x, masks, p):
    """Per site (0, 1): the smallest |y| in float64, ATen fp32's max |y32 - y64| on the same run, and the number of positions where the two
    disagree on the gate."""
    _threads()
    y64, y32 = pre_relu(sd, x, masks, p), pre_relu(sd, x, masks, p, dtype=torch.float32)
    return Margin(tuple(float(a.abs().min()) for a in y64),
                  tuple(float((b.double() - a).abs().max()) for a, b in zip(y64, y32)),
                  tuple(int(((b > 0) != (a > 0)).sum()) for a, b in zip(y64, y32)))


@functools.lru_cache(maxsize=None)
def case(name):
    """(geometry, (sd, x, x1, masks, targets, input lengths, target lengths)) with the gates cleared, once per case."""
    c = CASES[name]
    geom = gc.geometry(c.geom)
    B, T, L, Lt = c.shape
    sd, x, x1, masks, tg, il, tl = gc.train_case(geom, c.seed, B, T, L, Lt, P_DROP)
    return geom, (clear_gates(sd, x, masks, P_DROP, c.window), x, x1, masks, tg, il, tl)


def scaled_distance(a, b):
    """max |a - b| over max(1, max |b|): the training tests' gradient distance."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max()) / max(1.0, float(np.abs(b).max()))


def held(key):
    """The tensors the gate-clear bound is for: the conv weights and the conv BatchNorms' weight and bias (a conv bias in front of a
    batch-statistics BatchNorm has a gradient of exactly zero: only smallness compares)."""
    return key.startswith("conv.") and not key.endswith("conv.bias")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 step, d_ATen): ref_port.train_step in float64, and per parameter the distance of ATen's fp32 run of the same step from
    it.  Once per case for every run of it; the arrays are shared, so nobody writes into them."""
    from oracle import ref_port
    _threads()
    _, inputs = case(name)
    ref = ref_port.train_step(*inputs, P_DROP, dtype=torch.float64)
    g32 = ref_port.train_step(*inputs, P_DROP, dtype=torch.float32)[2]
    return ref, {k: scaled_distance(g32[k], ref[2][k]) for k in ref[2]}


def rounding_response(name, delta=2.0 ** -24):
    """How far one fp32 rounding of the parameters moves the float64 step: every float parameter times (1 + delta N(0,1)), the worst
    gradient distance from the unperturbed step, in the tests' scale.  The condition number of the draw as far as the bounds see it:
    7e-7 .. 1.5e-6 for the cases of the table; a draw of rnns.0's recurrence that answers with 1.4e-5 exists (see "last_direct")."""
    from oracle import ref_port
    _threads()
    _, inputs = case(name)
    rng = np.random.Generator(np.random.PCG64(1))
    sd = type(inputs[0])((k, v.astype(np.float64) * (1.0 + delta * rng.standard_normal(v.shape)) if v.dtype.kind == "f" and "running_" not in k else v)
                         for k, v in inputs[0].items())
    moved, grads = ref_port.train_step(sd, *inputs[1:], P_DROP, dtype=torch.float64)[2], reference(name)[0][2]
    return max(scaled_distance(moved[k], grads[k]) for k in grads if not k.endswith("conv.bias"))


def bound(name, key):
    """max(2e-5, 4 d_ATen) of scale: the project's bound outside the CNN, or four times ATen's own distance on this tensor of this case
    (the rule of tests/test_batch_tiles.py).  Nothing in it is measured on the code under test."""
    return max(2e-5, 4.0 * reference(name)[1][key])
