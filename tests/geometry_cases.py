"""The model geometries the suite runs beyond synth.REFERENCE / REFERENCE_256 / TINY, shared by tests/test_geometry.py (decode forward),
tests/test_train_geometry.py (training step) and tests/test_geometry_reference.py (the CPU side of both tables).

DECODE maps a name to (Geometry kwargs over the reference's defaults, expected plan).  The expected plan is written down by hand from
csrc/plan.h (plan_forward on a device that holds every persistent grid, no environment switch) and says, per requested precision, what
HipModel.precision and HipModel.profile must report:

    (precision in effect, conv front end, recurrence)
    conv front end   "fused": one conv_fused stage            "sep": conv0 + conv1
    recurrence       "layer": one persistent launch per BiLSTM  "step": one launch per time step

The rules behind the entries:
  * modes 1 / 2 need channels * W2, (mode 2) 2H and emb_dim to be multiples of 32, mode 1 also H in {256, 384}; mode 0 otherwise
  * the fused front end needs mode 1 or 2 in effect, feat = 243 and 32 channels
  * a persistent layer launch needs H in {256, 384} (and B <= 1024)
tests/test_geometry_reference.py::test_expected_plans_follow_plan_h builds plan.h with the host compiler and compares, so a change of the
policy fails there (on any machine) as well as in the GPU tests that read the observables."""
import numpy as np

from ctc_attention_mispronunciation_amd import synth

PRECISIONS = ("f32", "f32x6", "bf16x3")
SMALL, WIDE = (3, 12, 5), (17, 8, 65)          # (B, T, L): the row-tile and L > 64 edges the other modules use


def _plan(f32, f32x6, bf16x3):
    return {"f32": f32, "f32x6": f32x6, "bf16x3": bf16x3}


# packed hidden size: every mode honoured; the front end fused only with feat = 243 in modes 1 / 2
FAST_SEP = _plan(("f32", "sep", "layer"), ("f32x6", "sep", "layer"), ("bf16x3", "sep", "layer"))
FAST_FUSED = _plan(("f32", "sep", "layer"), ("f32x6", "fused", "layer"), ("bf16x3", "fused", "layer"))
# unpacked hidden size with 2H % 32 == 0: mode 2 for the projections, per-step recurrence; mode 1 falls back
STEP_SEP = _plan(("f32", "sep", "step"), ("f32x6", "sep", "step"), ("f32", "sep", "step"))
STEP_FUSED = _plan(("f32", "sep", "step"), ("f32x6", "fused", "step"), ("f32", "sep", "step"))
# a contraction length that is no multiple of 32: mode 0 whatever is asked
EXACT_LAYER = _plan(("f32", "sep", "layer"), ("f32", "sep", "layer"), ("f32", "sep", "layer"))
EXACT_STEP = _plan(("f32", "sep", "step"), ("f32", "sep", "step"), ("f32", "sep", "step"))

DECODE = {
    # ---- unfused conv into the fast GEMMs
    "feat120_H384_L4": (dict(feat=120), FAST_SEP),                                   # W1 = 60, W2 = 30
    "feat81_H256_L2": (dict(feat=81, hidden=256, layers=2), FAST_SEP),               # W1 = 41, W2 = 21: odd pair count in conv1_kernel
    "feat300_H256_L1": (dict(feat=300, hidden=256, layers=1), FAST_SEP),             # W1 = 150: two x-blocks of conv0_kernel
    "feat3_H64_L1": (dict(feat=3, hidden=64, layers=1), STEP_SEP),                   # W1 = 2, W2 = 1: K0 = 32, one K-tile
    "feat4_H64_L1": (dict(feat=4, hidden=64, layers=1), STEP_SEP),
    # ---- depth
    "H384_L1": (dict(layers=1), FAST_FUSED),
    "H256_L1": (dict(hidden=256, layers=1), FAST_FUSED),
    "H256_L2": (dict(hidden=256, layers=2), FAST_FUSED),
    "H256_L3": (dict(hidden=256, layers=3), FAST_FUSED),
    "H256_L5": (dict(hidden=256, layers=5), FAST_FUSED),
    "H256_L6": (dict(hidden=256, layers=6), FAST_FUSED),
    # ---- unpacked hidden sizes (J = 4H / 64 = 4, 8, 20, 32 in the matrix-core tail)
    "H64_L2": (dict(hidden=64, layers=2), STEP_FUSED),
    "H128_L2": (dict(hidden=128, layers=2), STEP_FUSED),
    "H320_L2": (dict(hidden=320, layers=2), STEP_FUSED),
    "H512_L2": (dict(hidden=512, layers=2), STEP_FUSED),
    "H48_ch4_feat39": (dict(feat=39, hidden=48, layers=2, channels=4), EXACT_STEP),  # K0 = 40; 4H = 192: the scalar tail
    "H20_ch4_feat39": (dict(feat=39, hidden=20, layers=2, channels=4), EXACT_STEP),  # H % 16 != 0: a ragged unit tile
    # ---- classes: 46..48 the last widths of the matrix-core tail's three tiles, 49 the first of the scalar tail, 65 / 101 past a wave
    "H256_L1_C2": (dict(hidden=256, layers=1, num_class=2, emb_rows=2), FAST_FUSED),
    "H256_L1_C46": (dict(hidden=256, layers=1, num_class=46), FAST_FUSED),
    "H256_L1_C47": (dict(hidden=256, layers=1, num_class=47), FAST_FUSED),
    "H256_L1_C48": (dict(hidden=256, layers=1, num_class=48), FAST_FUSED),
    "H256_L1_C49": (dict(hidden=256, layers=1, num_class=49), FAST_FUSED),
    "H256_L1_C64": (dict(hidden=256, layers=1, num_class=64), FAST_FUSED),
    "H256_L1_C65": (dict(hidden=256, layers=1, num_class=65), FAST_FUSED),
    "H256_L1_C101": (dict(hidden=256, layers=1, num_class=101), FAST_FUSED),
    "H384_L1_C49": (dict(layers=1, num_class=49), FAST_FUSED),
    # ---- embedding
    "H256_L1_E300": (dict(hidden=256, layers=1, emb_dim=300), EXACT_LAYER),          # 300 % 32 != 0 drops the whole model to mode 0
    "H256_L1_E64": (dict(hidden=256, layers=1, emb_dim=64), FAST_FUSED),
    "H256_L1_E32": (dict(hidden=256, layers=1, emb_dim=32), FAST_FUSED),             # one K-tile in the text table's GEMM
    "H256_L1_C101_rows100": (dict(hidden=256, layers=1, num_class=101, emb_rows=100), FAST_FUSED),
    "H256_L1_rows1": (dict(hidden=256, layers=1, emb_rows=1), FAST_FUSED),           # every id 0
}

# The three mid geometries of the other entry points (forward_raw, forward_fused) and the two of the canonical-length limit.
MID = ("feat120_H384_L4", "H128_L2", "H256_L1_C49")
LIMIT = {"H128_L2": 2364 - 2 * 128, "H128_L2_C49": 2560 - 4 * 128 - 49}     # matrix-core tail: 2108; scalar tail: 1999
DECODE_LIMIT_EXTRA = {"H128_L2_C49": (dict(hidden=128, layers=2, num_class=49), STEP_FUSED)}

# Training: name -> (Geometry kwargs, modes).  Every case runs "f32"; "f32x6" where at least one contraction of the step passes gemm_big's
# size rule at the shapes below (M, N >= 128, K >= 64, M.N.K >= 2^27: csrc/train.hip) and on "H64_L2" where none does (G2 = 512, K <= 960,
# 64 rows: 3.1e7 multiply-adds), which must then meet mode 0's bounds through the fallback.  "bf16x3" on H = 64: no persistent kernel is
# built for it and no contraction reaches the variant's thresholds, so the step is mode 0's.
TRAIN_SHAPES = ((4, 32, 6), (5, 16, 3))         # (B, T, L): B * T >= 64, so the batch statistics are well conditioned
TRAIN = {
    "feat120_H64_L2_C20": (dict(feat=120, hidden=64, layers=2, num_class=20, emb_rows=19, emb_dim=64), ("f32", "f32x6", "bf16x3")),
    "feat300_H256_L1": (dict(feat=300, hidden=256, layers=1), ("f32", "f32x6")),    # W1 = 150 > 128: conv1 through im2col, switch unset
    "feat39_H20_ch4_C12": (dict(feat=39, hidden=20, layers=2, channels=4, num_class=12, emb_rows=11, emb_dim=20), ("f32",)),
    "H256_L1": (dict(hidden=256, layers=1), ("f32", "f32x6")),
    "H256_L5": (dict(hidden=256, layers=5), ("f32", "f32x6")),
    "H256_L1_C49": (dict(hidden=256, layers=1, num_class=49), ("f32", "f32x6")),
    "H256_L1_C101": (dict(hidden=256, layers=1, num_class=101), ("f32", "f32x6")),
}


def geometry(kwargs):
    return synth.Geometry(**dict(synth.REFERENCE, **kwargs))


def decode_geometry(name):
    return geometry((DECODE.get(name) or DECODE_LIMIT_EXTRA[name])[0])


def draw_batch(geom, B, T, L, seed):
    """synth.synth_batch's features and ragged lengths with the ids drawn here: uniform over the WHOLE table [0, emb_rows), the last row
    (emb_rows - 1) present in every batch, whatever num_class is (synth_batch cannot draw when min(emb_rows, C - 1) <= 2)."""
    rng = np.random.Generator(np.random.PCG64(seed + 17))
    x = rng.standard_normal((B, T, geom.feat)).astype(np.float32)
    x1 = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        lb = L if b == 0 else int(rng.integers(max(1, L // 2), L + 1))
        x1[b, :lb] = rng.integers(0, geom.emb_rows, size=lb)
        if b > 0:
            tb = int(rng.integers(T // 2, T + 1))
            tb -= tb % 2
            x[b, tb:, :] = 0.0
    x1[0, L - 1] = geom.emb_rows - 1
    return x, x1


def train_case(geom, seed, B, T, L, Lt=4, p=0.2):
    """synth.train_case with the canonical ids drawn by draw_batch (emb_rows = 11 / 19 / 44 against C = 12 / 20 / 101)."""
    sd, x, _, masks, tg, il, tl = synth.train_case(geom, seed, B, T, L, Lt, p)
    _, x1 = draw_batch(geom, B, T, L, seed)
    return sd, x, x1, masks, tg, il, tl


def reference_scores(taps, layers):
    """The attention scores [B, T', L] of the float64 taps (queries: the last BiLSTM layer's raw output)."""
    return np.einsum("tbd,lbd->btl", taps["rnn%d" % (layers - 1)], taps["key"])
