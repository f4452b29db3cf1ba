"""The batch-tile geometries of the persistent BiLSTM layer kernels, shared by tests/test_batch_tiles.py (decode forward, GPU),
tests/test_train_batch_tiles.py (training step, GPU) and tests/test_batch_tiles_reference.py (the CPU side of both).  No tests in here.

The three layer kernels pick a template instantiation from the batch size (csrc/plan.h, lstm_granule.hip, lstm_f32.hip, lstm_x6.hip):

    lstm_layer_x6_kernel<H, NBT>            128 rows per tile   NBT = ceil(ceil(B / 8) / 16) = 1..8    (NBT >= 3: the skewed schedule)
    lstm_layer_f32_kernel<H, NBT>           256 rows per tile   NBT = team8_tiles(B)          = 1..4
    lstm_layer_granule_kernel<H, NBT, RTW>  256 rows per tile   NBT = team8_tiles(B)          = 1..4

TILE_B holds the first batch of each x6 instantiation NBT = 2..8 (one row into a new tile) and the full B = 1024; NBT is written down by
hand from the formulas and compared with plan.h by tests/test_batch_tiles_reference.py.  B = 17 (one tile, held to float64 by
tests/test_geometry.py) and B = 1025 (past kPersistMaxB: no layer kernel, one launch per step) complete the table."""
import functools

import numpy as np
import torch

from tests import geometry_cases as gc
from ctc_attention_mispronunciation_amd import synth

HIDDEN = (384, 256)
PRECISIONS = gc.PRECISIONS                      # ("f32", "f32x6", "bf16x3")
TILE_B = (129, 257, 385, 513, 641, 769, 897, 1024)
PAST_B = 1025                                   # the first batch past kPersistMaxB
SHORT = (12, 6)                                 # (T, L) of every TILE_B case: T' = 6
LONG = (384, 300, 120, 9)                       # (H, B, T, L): T' = 60 on x6 NBT = 3 (skewed) and granule / f32 NBT = 2

# B -> (x6 NBT, granule and f32 NBT); None: no persistent layer kernel at this batch
NBT = {
    17: (1, 1),
    129: (2, 1),
    257: (3, 2),
    300: (3, 2),
    385: (4, 2),
    513: (5, 3),
    641: (6, 3),
    769: (7, 4),
    897: (8, 4),
    1024: (8, 4),
    1025: (None, None),
}

# The layer kernel the library's own choice gives (hidden, requested precision) at a batch past 128 rows (plan_forward: the f32x6 teams at
# H = 384 for every batch, at H = 256 up to 128 rows only); MDD_LSTM_X6=force gives "x6" at H = 256 too.
LAYER_KERNEL = {
    (384, "f32"): "f32", (384, "f32x6"): "x6", (384, "bf16x3"): "granule",
    (256, "f32"): "f32", (256, "f32x6"): "f32", (256, "bf16x3"): "granule",
}

# Training step (H, B, T, L), each in both train_precision modes: bilstm_forward takes the persistent TRAIN layer kernel of the variant for
# B <= 512 (NBT = 1 up to 256 rows, 2 beyond), lstm_backward the persistent BPTT kernel for B <= 256 (csrc/train.hip).
TRAIN_SHAPES = (
    (384, 256, 8, 3),       # last batch of the persistent BPTT kernel; forward NBT = 1 with full rows
    (384, 257, 8, 3),       # first batch of lstm_layer_granule_kernel<384, 2, 3, true>; per-step backward
    (384, 512, 8, 3),       # last batch of the persistent TRAIN forward
    (384, 513, 8, 3),       # the variant's fall-back to the per-step forward
    (256, 256, 8, 3),       # last batch of the persistent BPTT kernel at H = 256
    (256, 513, 8, 3),       # the variant's fall-back at H = 256
)
TRAIN_MODES = ("f32", "bf16x3")
TRAIN_PERSIST_MAX_B = 512


def geometry(hidden):
    return synth.Geometry(**dict(synth.REFERENCE, hidden=hidden))


@functools.lru_cache(maxsize=None)
def state_dict(hidden):
    return synth.synth_state_dict(geometry(hidden), seed=77)


def tap_names(geom):
    """In forward order."""
    return ["conv1"] + ["rnn%d" % i for i in range(geom.layers)] + ["text", "key", "score"]


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)


def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


# Two entries: the precisions of one (H, B) run back to back (the innermost parameter), and a B = 1024 case holds ~0.3 GB of float64 taps.
@functools.lru_cache(maxsize=2)
def case(hidden, B, T=SHORT[0], L=SHORT[1]):
    """(x, x1, float64 log-probs, float64 taps with "score"): computed once per shape, shared by every precision and switch."""
    from oracle import ref_port
    _threads()
    geom = geometry(hidden)
    x, x1, _, _ = synth.synth_batch(geom, B, T=T, L=L, seed=B, ragged=True)
    taps = {}
    logp = ref_port.forward(state_dict(hidden), x, x1, dtype=torch.float64, taps=taps).numpy()
    assert logp.dtype == np.float64
    taps["score"] = gc.reference_scores(taps, geom.layers)
    _freeze([x, x1, logp] + list(taps.values()))
    return x, x1, logp, taps


@functools.lru_cache(maxsize=2)
def aten_fp32_distance(hidden, B, T=SHORT[0], L=SHORT[1]):
    """{"logp" | tap: max |ATen fp32 - float64|} of the same case: what the reference's own arithmetic is away from the yardstick."""
    from oracle import ref_port
    _threads()
    x, x1, logp, taps = case(hidden, B, T, L)
    t32 = {}
    l32 = ref_port.forward(state_dict(hidden), x, x1, taps=t32).numpy()
    assert l32.dtype == np.float32
    d = {k: float(np.abs(v.astype(np.float64) - taps[k]).max()) for k, v in t32.items()}
    d["logp"] = float(np.abs(l32.astype(np.float64) - logp).max())
    return d


@functools.lru_cache(maxsize=2)
def train_case(hidden, B, T, L):
    """(geometry, inputs of synth.train_case, the float64 step of oracle/ref_port.train_step), once per shape for both modes."""
    from oracle import ref_port
    _threads()
    geom = geometry(hidden)
    inputs = synth.train_case(geom, 77, B, T, L, max(1, min(6, T // 4)))
    _freeze([a for a in inputs[1:3]] + list(inputs[3]) + list(inputs[4:]))
    return geom, inputs, ref_port.train_step(*inputs, 0.2, dtype=torch.float64)
