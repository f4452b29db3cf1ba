"""Every kernel path of csrc/greedy.hip and csrc/beam*.hip against the CPU oracle (oracle/mdd_oracle.c: orc_beam / orc_greedy), through the C ABI.

The three search kernels and the host dispatch are driven with any class count, beam width, blank index and batch size: several waves
per workgroup (B > 64, MDD_BEAM_W), both fast-kernel instantiations and their slot-count edges, the same shapes through the generic
kernel (MDD_BEAM_GENERIC), the generic-only shapes (beam > 16, C > 64, C < beam, LM table in LDS and in HBM), prefix rows longer than
64 words, exact ties (the reference's dict-insertion order decides), the first-error order, the LDS limits of the host dispatch, and
the greedy kernel's lane-stride loop, tie rule and compaction.

What a beam comparison asserts: ids, nids and status equal the oracle's for every utterance; scores of status-0 rows within 1e-7
relative (the two sides round exp(logp) to fp32 with different libm's, see test_gpu_parity.test_decoders_full_size_against_oracle);
the score of an error row is NaN; every output entry was written (sentinel prefill).

Robustness (CPU): the oracle uses expf, the GPU a correctly rounded exp, so a case whose winner hangs on one ulp of exp() proves
nothing.  Every case must therefore decode identically in the C oracle and in the Python dict port (oracle/ref_port.py: torch.exp and
math.log); a case that does not gets another seed, never a skip.

Known blind spots.  Which of the two slots a merged entry occupies (`q < a` in the kernels) moves it only in the insertion order: on
the symmetric ties of the tied and uniform families both placements sort alike, so only the hand-built `mergetie` family (a merged
entry that ties a non-mate at the cut of the beam) tells them apart.  The environment switches cannot be observed through the ABI: if
the library stopped reading MDD_BEAM_W or MDD_BEAM_GENERIC, the routes would run one kernel and still pass.  The prefix-verify loop
matters only on a hash collision, which nothing here injects.

The LDS limits restated below in Python are csrc/plan.h's beam_plan, which tests/test_beam_plan_host.py walks on the CPU; the stamped
instantiations of the single-wave kernel run through mdd_diag_beam_stamps at the end of the beam section."""
import ctypes as C
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

from oracle import oracle
from ctc_attention_mispronunciation_amd import synth

SCORE_RTOL = 1e-7          # the bound of test_decoders_full_size_against_oracle
MDD_OK, MDD_ERR_ARG = 0, -1
SENT_I, SENT_F = -77, 12345.5
KB = 1024


# ------------------------------------------------------------------------------------------------------------ inputs
class Case(NamedTuple):
    name: str
    family: str              # flat | peaky | tied | uniform | errors
    C: int
    beam: int
    blank: int
    alpha: float
    T: int
    B: int
    seed: int
    lens: Optional[Tuple[int, ...]] = None      # None: every utterance has T frames; "ragged" families fill their own
    ragged: bool = False
    routes: Tuple[str, ...] = ("auto",)         # auto | generic (MDD_BEAM_GENERIC=1) | w2 | w3 (MDD_BEAM_W)
    port_rows: Optional[int] = None             # rows the pure-Python port decodes (None: all)
    min_ids: int = 0                            # the oracle's winner of row 0 must be longer than this (long-prefix cases)


def _log_softmax(z):
    return torch.log_softmax(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)), -1).numpy()


def fast_eligible(beam, Cn):
    """The host's choice (mdd_beam): the single-wave kernel takes beam <= 16, C <= 64, beam*C <= 1024."""
    return beam <= 16 and Cn <= 64 and beam * Cn <= 1024


# rows of the `errors` family, by b % 12, and the status the reference's execution order gives each (0 ok, 1 IndexError,
# 2 ValueError, 3 KeyError).  p1: a class whose LM row holds a NaN at column q1 (KeyError as soon as a kept beam ends in p1 and is
# extended); p2: a class whose end-of-sentence cell is NaN; a: an ordinary class; kz_lo < q1 < kz_hi: classes whose posterior is
# zeroed (exp(-120) == 0 in fp32: ValueError).  p1 and p2 are 40 nats down everywhere else, so no other row ever keeps them.
ERROR_ROWS = (
    ("clean", 0),
    ("key_rank0", 3),                 # the best beam ends in p1: KeyError at (rank 0, q1)
    ("value_before_key", 2),          # same frame, same beam: the zero at kz_lo < q1 is met first
    ("key_before_value", 3),          # same frame, same beam: the zero at kz_hi > q1 is met after the NaN
    ("value_rank0_key_lower", 2),     # the p1 beam ranks below the best: (rank 0, kz_hi) precedes (rank r, q1)
    ("value_on_last_symbol", 2),      # the copy path of a beam whose last id has probability 0
    ("value_on_blank", 2),            # p(blank) == 0: the copy path of rank 0
    ("all_blank", 1),                 # every frame skipped: the empty prefix is the only final beam
    ("len0", 1),
    ("key_at_eos", 3),                # the best final beam ends in p2
    ("clean_short", 0),
    ("key_lower_beam", 3),            # KeyError met in a beam of rank > 0, nothing before it
)


def _error_classes(Cn, blank):
    nbk = [k for k in range(Cn) if k != blank]
    n = len(nbk)
    return dict(p1=nbk[n // 3], p2=nbk[(2 * n) // 3], q1=nbk[n // 2], kz_lo=nbk[1], kz_hi=nbk[n - 2], a=nbk[3])


def _errors_family(case, rs):
    T, B, Cn, blank = case.T, case.B, case.C, case.blank
    k = _error_classes(Cn, blank)
    tK = 6
    z = rs.standard_normal((T, B, Cn))
    z[..., k["p1"]] -= 40.0
    z[..., k["p2"]] -= 40.0
    lens = np.full(B, T, dtype=np.int32)
    zero = []                                       # (t, b, class) posteriors set to exp(-120) after the softmax
    for b in range(B):
        kind = ERROR_ROWS[b % len(ERROR_ROWS)][0]
        if kind in ("key_rank0", "value_before_key", "key_before_value"):
            z[tK, b, k["p1"]] = 12.0
            if kind == "value_before_key":
                zero.append((tK + 1, b, k["kz_lo"]))
            if kind == "key_before_value":
                zero.append((tK + 1, b, k["kz_hi"]))
        elif kind in ("value_rank0_key_lower", "key_lower_beam"):
            z[0, b, k["a"]] = 12.0                  # on the first frame the ranks are certain: (a) is rank 0, (p1) is rank 1
            z[0, b, k["p1"]] = 11.5
            if kind == "value_rank0_key_lower":
                zero.append((1, b, k["kz_hi"]))
        elif kind == "value_on_last_symbol":
            z[tK, b, k["a"]] = 12.0
            zero.append((tK + 1, b, k["a"]))
        elif kind == "value_on_blank":
            zero.append((tK, b, blank))
        elif kind == "all_blank":
            z[:, b, blank] += 40.0
        elif kind == "len0":
            lens[b] = 0
        elif kind == "key_at_eos":
            z[T - 1, b, k["p2"]] = 12.0
        elif kind == "clean_short":
            lens[b] = T // 2
    logp = _log_softmax(z)
    for t, b, c in zero:
        logp[t, b, c] = -120.0
    return logp, lens, k


def _merge_tie_logp(blank):
    """Hand-built (C 4, beam 3, T 5): a merged entry ties an entry that is not its symmetric mate, at the cut of the beam.
    k1 < k2 are mates (equal on every frame), k3 is a third class.  Frame 0 keeps (), (k3), (k1): (k1) and (k2) tie 50 nats down and
    k1 is inserted first.  On frame 1 the extension () + k1 merges with the copy of beam (k1), which lies 48 nats below it, so the
    sum IS the extension's value (1 + exp(-48) == 1 in fp64), exactly the value of the unmerged () + k2.  The reference keeps the
    dict entry where it was inserted first, () + k1 at (rank 0, k1), ahead of (rank 0, k2), so (k1) takes the third place and the
    winner starts with k1; an entry placed at the copy slot of rank 2 instead loses the place to (k2), and the winner starts with k2."""
    k1, k2, k3 = [k for k in range(4) if k != blank]
    tiny = np.exp(-50.0)
    rows = [(0.5, tiny, tiny, 0.4), (0.5, 0.25, 0.25, tiny)] + [(0.02, 0.49, 0.49, tiny)] * 3
    logp = np.zeros((len(rows), 4), dtype=np.float32)
    for t, r in enumerate(rows):
        logp[t, [blank, k1, k2, k3]] = np.log(r).astype(np.float32)
    return logp


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(logp [T,B,C] float32, lens int32 [B], LM table float64 [(C+1),(C+1)]) of a case; built once and never modified."""
    rs = np.random.Generator(np.random.PCG64(case.seed))
    T, B, Cn, blank = case.T, case.B, case.C, case.blank
    lm = np.log(rs.uniform(0.01, 1.0, size=(Cn + 1, Cn + 1)))
    lens = np.full(B, T, dtype=np.int32)
    if case.family == "flat":
        logp = _log_softmax(rs.standard_normal((T, B, Cn)))
    elif case.family == "peaky":
        logp = np.stack([synth.peaky_logp(T, Cn, max(1, T // 8), seed=case.seed * 1000 + b) for b in range(B)], axis=1)
        if blank != 0:                              # peaky_logp boosts class 0 as the blank
            logp[..., [0, blank]] = logp[..., [blank, 0]]
    elif case.family == "tied":
        G = max(2, Cn // 4)
        group = rs.permutation(Cn) % G              # the fixed class -> group map
        z = rs.standard_normal((T, B, G))[..., group]
        z[..., blank] -= 0.5
        logp = _log_softmax(z)
        for g in range(G):                          # the family's premise: group mates are bit-identical on every frame
            members = np.nonzero((group == g) & (np.arange(Cn) != blank))[0]
            assert (logp[..., members] == logp[..., members[:1]]).all()
    elif case.family == "uniform":
        logp = _log_softmax(np.zeros((T, B, Cn)))
    elif case.family == "mergetie":
        logp = np.repeat(_merge_tie_logp(blank)[:, None, :], B, axis=1)
    elif case.family == "errors":
        logp, lens, k = _errors_family(case, rs)
        lm[k["p1"], k["q1"]] = np.nan
        lm[k["p2"], Cn] = np.nan
    else:
        raise AssertionError(case.family)
    if case.lens is not None:
        lens = np.asarray(case.lens, dtype=np.int32)
    elif case.ragged:
        lens = rs.integers(2, T + 1, size=B).astype(np.int32)
        lens[[0, 1, 2, 3]] = (T, 0, 1, T + 50)
        lens[B - 1] = T                             # the last wave of the last workgroup decodes a whole utterance
    assert lens.shape == (B,)
    for a in (logp, lens, lm):
        a.setflags(write=False)
    return logp, lens, lm


@functools.lru_cache(maxsize=None)
def expected(case):
    """The oracle's answer: (list of id lists, status [B], score [B]).  Computed once per case, shared by every route."""
    logp, lens, lm = inputs(case)
    want, st, sc = oracle.beam(logp, lens, lm, beam_width=case.beam, alpha=case.alpha, blank=case.blank, return_scores=True)
    st.setflags(write=False)
    sc.setflags(write=False)
    return want, st, sc


def _cases():
    out = []
    # 1. workgroup packing: B > 64 puts W = 2..4 waves (utterances) in a workgroup; the last group is partly empty
    for B, fam, seed in ((65, "flat", 11), (66, "errors", 12), (130, "tied", 13)):
        out.append(Case("pack_B%d_%s" % (B, fam), fam, 45, 10, 0, 0.0 if fam == "tied" else 0.2, 24, B, seed, ragged=fam != "errors",
                        routes=("auto", "w2", "w3"), port_rows=12 if fam == "errors" else 4))
    # 2./3. both instantiations of the fast kernel (NS 8: beam*C <= 512, NS 16: <= 1024), their edges, and the generic kernel on
    # the same inputs
    for beam, Cn in ((8, 64), (9, 57), (16, 45), (16, 64), (1, 2), (16, 2), (3, 64)):
        for blank in sorted({0, Cn // 2, Cn - 1}):
            for fam in ("flat", "tied"):
                out.append(Case("fast_%s_b%d_C%d_blank%d" % (fam, beam, Cn, blank), fam, Cn, beam, blank, 0.2 if fam == "flat" else 0.0,
                                40, 3, 100 + beam + Cn + blank, lens=(40, 33, 17), routes=("auto", "generic")))
    # 4. generic only: beam > 16 or C > 64 (up to four classes per lane), C < beam (fewer finite lane maxima than beams to
    # keep), LM table in LDS ((64, 45, 40)) and read from HBM ((64, 45, 200), C >= 100)
    for beam, Cn, T in ((17, 45, 40), (64, 45, 40), (64, 45, 200), (16, 65, 30), (40, 100, 30), (8, 256, 20), (64, 3, 30), (64, 9, 30)):
        for alpha in (0.0, 0.25):
            for blank in (0, Cn - 1) if (beam, Cn) in ((16, 65), (8, 256), (64, 3)) else (0,):
                out.append(Case("generic_b%d_C%d_T%d_a%g_blank%d" % (beam, Cn, T, alpha, blank), "flat", Cn, beam, blank, alpha, T, 2,
                                200 + beam + Cn + T, lens=(T, T // 2 - 3)))
    # 5. prefix rows longer than 64 words (T > 252): the second pass of the prefix verify and copy loops
    for T in (253, 300, 520):
        for beam in (10, 16, 20):
            out.append(Case("long_T%d_b%d" % (T, beam), "flat", 45, beam, 0, 0.0, T, 2, 300 + T + beam, lens=(T, 255),
                            min_ids=256 if T >= 300 else 0))
    out.append(Case("long_T300_b16_C64_blank63", "flat", 64, 16, 63, 0.0, 300, 2, 364, lens=(300, 255), min_ids=256))
    # 6. exact ties: the insertion order (copy first, then k ascending, then beam rank) decides, in both kernels
    out += [Case("tie_tied_b16_C12_blank5_a0", "tied", 12, 16, 5, 0.0, 40, 3, 401, lens=(40, 31, 8), routes=("auto", "generic")),
            Case("tie_tied_b16_C12_blank5_a0.3", "tied", 12, 16, 5, 0.3, 40, 3, 402, lens=(40, 31, 8)),
            Case("tie_tied_b10_C45", "tied", 45, 10, 0, 0.0, 60, 3, 403, lens=(60, 47, 9), routes=("auto", "generic")),
            Case("tie_tied_b16_C45_blank44", "tied", 45, 16, 44, 0.25, 60, 3, 404, lens=(60, 47, 9)),
            Case("tie_tied_b40_C45", "tied", 45, 40, 0, 0.0, 30, 3, 405, lens=(30, 22, 9)),
            Case("tie_uniform_b10_C9", "uniform", 9, 10, 0, 0.0, 20, 2, 406, lens=(20, 13)),
            Case("tie_uniform_b10_C45", "uniform", 45, 10, 0, 0.0, 20, 2, 407, lens=(20, 13), routes=("auto", "generic")),
            Case("tie_uniform_b16_C45_blank7", "uniform", 45, 16, 7, 0.0, 20, 2, 408, lens=(20, 13)),
            Case("tie_uniform_b16_C12_blank5", "uniform", 12, 16, 5, 0.0, 20, 2, 409, lens=(20, 13)),
            Case("tie_uniform_b40_C45", "uniform", 45, 40, 0, 0.0, 20, 2, 410, lens=(20, 13))]
    out += [Case("tie_merge_blank%d" % bl, "mergetie", 4, 3, bl, 0.0, 5, 2, 420 + bl, routes=("auto", "generic")) for bl in (0, 1, 3)]
    # 7. the first error in the reference's execution order, on the generic kernel (lanes own classes, beams are a loop) and on
    # the fast one (lanes own slots)
    out += [Case("errors_b20_C45", "errors", 45, 20, 0, 0.2, 24, 12, 501),
            Case("errors_b8_C100", "errors", 100, 8, 0, 0.2, 24, 12, 502),
            Case("errors_b10_C45", "errors", 45, 10, 0, 0.2, 24, 12, 503, routes=("auto", "generic"))]
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------- the host's LDS limits, restated
def _tcap(T):
    return (T + 1 + 3) & ~3                         # a prefix row: T ids + 1, in whole words


def generic_lds_bytes(beam, Cn, T):
    """beam_kernel: candidate totals, compacted values (fp64) and orders (int) per slot, the frame flags and two sets of `beam`
    prefix rows; the LM table joins them in LDS while the sum stays within 96 KB.  Accepted up to 140 KB."""
    base = (8 * 2 + 4) * beam * Cn + (2 * beam + 1) * _tcap(T)
    lm = 8 * (Cn + 1) * (Cn + 1)
    return base + (lm if base + lm <= 96 * KB else 0)


def fast_lds_bytes(beam, Cn, T):
    """beam_fast_kernel with one wave: the LM table, NS*64 slots (value, compacted value, order, slot index), the beam state of 16
    beams, the frame flags and two sets of 16 prefix rows.  Accepted up to 160 KB."""
    NS, FB = (8 if beam * Cn <= 512 else 16), 16
    wave = 8 * (2 * NS * 64 + 64 + 10 * FB) + 8 * 4 * FB + 4 * (2 * NS * 64 + 6 * FB) + (2 * FB + 1) * _tcap(T)
    lm = (8 * (Cn + 1) * (Cn + 1) + 15) & ~15
    return lm + ((wave + 15) & ~15)


def beam_accepts(beam, Cn, T):
    if generic_lds_bytes(beam, Cn, T) > 140 * KB:
        return False
    return not fast_eligible(beam, Cn) or fast_lds_bytes(beam, Cn, T) <= 160 * KB


def beam_max_T(beam, Cn):
    T = 1
    while beam_accepts(beam, Cn, T + 1):
        T += 1
    assert beam_accepts(beam, Cn, T) and not any(beam_accepts(beam, Cn, T + d) for d in range(1, 9))
    return T


LIMIT_SHAPES = ((10, 45), (64, 45))
GREEDY_MAX_T = 150 * KB // 4                       # one int of LDS per frame


def limit_case(beam, Cn):
    T = beam_max_T(beam, Cn)
    return Case("limit_b%d_C%d_T%d" % (beam, Cn, T), "peaky", Cn, beam, 0, 0.0, T, 1, 600 + beam)


def test_limit_formulas_give_the_documented_bounds():
    """include/mdd_hip.h states these two numbers for the reference's 45 classes."""
    assert beam_max_T(10, 45) == 3995 and beam_max_T(64, 45) == 663


# ------------------------------------------------------------------------------------------- robustness (CPU, no GPU)
class _TableLM:
    """The LanguageModel interface ref_port.beam needs, backed by the dense table ("" = sentence start / end, NaN = KeyError)."""

    def __init__(self, table):
        self.table, self.C = table, table.shape[0] - 1

    def get_bi_prob(self, w1, w2):
        v = self.table[int(w1) if w1 != "" else self.C, int(w2) if w2 != "" else self.C]
        if v != v:
            raise KeyError((w1, w2))
        return float(v)


def _port_beam(case, rows):
    from oracle import ref_port
    logp, lens, lm = inputs(case)
    i2c = {k: str(k) for k in range(case.C)}
    ids, status = [], []
    for b in range(rows):
        try:
            s = ref_port.beam(logp[:, b:b + 1].copy(), [min(int(lens[b]), case.T)], i2c, _TableLM(lm), case.beam, case.alpha, case.blank)[0]
            ids.append([int(w) for w in s.split(" ")])
            status.append(0)
        except (IndexError, ValueError, KeyError) as e:
            ids.append([])
            status.append({IndexError: 1, ValueError: 2, KeyError: 3}[type(e)])
    return ids, status


def _check_robust(case):
    want, st, _ = expected(case)
    rows = case.B if case.port_rows is None else min(case.port_rows, case.B)
    ids, status = _port_beam(case, rows)
    assert status == st[:rows].tolist(), case.name
    assert ids == want[:rows], case.name
    if case.min_ids:
        assert len(want[0]) > case.min_ids, (case.name, len(want[0]))
    if case.family == "errors":
        assert st.tolist() == [ERROR_ROWS[b % len(ERROR_ROWS)][1] for b in range(case.B)], case.name


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_and_python_port_agree(name):
    _check_robust(CASE_BY_NAME[name])


@pytest.mark.parametrize("beam,Cn", LIMIT_SHAPES)
def test_oracle_and_python_port_agree_at_the_T_limit(beam, Cn):
    _check_robust(limit_case(beam, Cn))


def test_error_rows_cover_every_status_and_both_orders():
    kinds = dict(ERROR_ROWS)
    assert set(kinds.values()) == {0, 1, 2, 3}
    assert kinds["value_before_key"] == 2 and kinds["key_before_value"] == 3 and kinds["value_rank0_key_lower"] == 2
    for name in ("errors_b20_C45", "errors_b8_C100", "errors_b10_C45", "pack_B66_errors"):
        c = CASE_BY_NAME[name]
        k = _error_classes(c.C, c.blank)
        assert k["kz_lo"] < k["q1"] < k["kz_hi"] and len(set(k.values())) == len(k) and c.blank not in k.values()
    k = _error_classes(100, 0)                       # C 100: the competing classes sit in different lanes and strides
    assert k["q1"] % 64 != k["kz_lo"] % 64 != k["kz_hi"] % 64 and k["kz_hi"] >= 64 > k["q1"]


# ------------------------------------------------------------------------------------ host refusals (CPU, no device work)
def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


_FAKE = 4096      # a non-NULL value for pointers that must never be dereferenced: every call below is refused on the host


def _beam_args(**over):
    a = dict(logp=_FAKE, T=10, B=2, C=45, len=_FAKE, beam=10, blank=0, lm=_FAKE, alpha=0.0, ids=_FAKE, nids=_FAKE, status=_FAKE,
             score=_FAKE)
    a.update(over)
    return (C.c_void_p(a["logp"]), a["T"], a["B"], a["C"], C.c_void_p(a["len"]), a["beam"], a["blank"], C.c_void_p(a["lm"]),
            C.c_double(a["alpha"]), C.c_void_p(a["ids"]), C.c_void_p(a["nids"]), C.c_void_p(a["status"]), C.c_void_p(a["score"]), None)


@pytest.mark.parametrize("over", [dict(beam=0), dict(beam=65), dict(C=1), dict(C=257), dict(blank=-1), dict(blank=45), dict(T=0),
                                  dict(B=0), dict(logp=None), dict(len=None), dict(lm=None), dict(ids=None), dict(nids=None),
                                  dict(status=None), dict(beam=64, C=45, T=664), dict(beam=64, C=256, T=30), dict(beam=20, C=45, T=3500)],
                         ids=lambda o: "_".join("%s=%s" % kv for kv in o.items()))
def test_beam_bad_arguments_are_refused_on_the_host(over):
    """None of these reaches a device call (this test runs without a GPU); the last three are LDS refusals of the generic kernel."""
    L = _L()
    assert L.mdd_beam(*_beam_args(**over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_beam"), msg
    if "T" in over and over["T"] > 0 or over.get("C") == 256:
        assert "LDS" in msg and not beam_accepts(over.get("beam", 10), over.get("C", 45), over.get("T", 10)), msg


@pytest.mark.parametrize("over", [dict(T=GREEDY_MAX_T + 1), dict(T=0), dict(B=0), dict(C=0), dict(blank=-1), dict(blank=45),
                                  dict(logp=None), dict(len=None), dict(ids=None), dict(nids=None)],
                         ids=lambda o: "_".join("%s=%s" % kv for kv in o.items()))
def test_greedy_bad_arguments_are_refused_on_the_host(over):
    a = dict(logp=_FAKE, T=10, B=2, C=45, len=_FAKE, blank=0, ids=_FAKE, nids=_FAKE)
    a.update(over)
    L = _L()
    rc = L.mdd_greedy(C.c_void_p(a["logp"]), a["T"], a["B"], a["C"], C.c_void_p(a["len"]), a["blank"], C.c_void_p(a["ids"]),
                      C.c_void_p(a["nids"]), None)
    assert rc == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_greedy"), msg
    if a["T"] > GREEDY_MAX_T:
        assert "T=%d" % a["T"] in msg, msg


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # a copy: the shared inputs are read-only


def _ptr(t):
    return C.c_void_p(t.data_ptr())


SPARE = 3      # rows past B in every per-utterance array: W - 1 waves of the last workgroup have b >= B


def gpu_beam(logp, lens, lm, beam, blank, alpha):
    """One mdd_beam call on sentinel-filled outputs: (rc, ids [B,T], nids, status, score) as numpy.
    A workgroup of the fast kernel holds up to four utterances, so up to three waves of the last one have b >= B and must return at
    once.  len, ids, nids, status and score therefore carry SPARE rows past B (a valid short length; sentinels): a wave that ran on
    would stay inside every array, the library's own scratch included, and leave its marks in rows that must come back untouched."""
    T, B, Cn = logp.shape
    lens_dev = np.concatenate([np.asarray(lens, dtype=np.int32), np.full(SPARE, min(T, 2), dtype=np.int32)])
    d_lp, d_len, d_lm = _dev(logp), _dev(lens_dev), _dev(np.asarray(lm, dtype=np.float64))
    ids = torch.full((B + SPARE, T), SENT_I, dtype=torch.int32, device="cuda")
    nids = torch.full((B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    st = torch.full((B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((B + SPARE,), SENT_F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_beam(_ptr(d_lp), T, B, Cn, _ptr(d_len), beam, blank, _ptr(d_lm), C.c_double(alpha), _ptr(ids), _ptr(nids), _ptr(st),
                       _ptr(sc), None)
    torch.cuda.synchronize()
    ids, nids, st, sc = ids.cpu().numpy(), nids.cpu().numpy(), st.cpu().numpy(), sc.cpu().numpy()
    assert (ids[B:] == SENT_I).all() and (nids[B:] == SENT_I).all() and (st[B:] == SENT_I).all() and (sc[B:] == SENT_F).all(), \
        "rows past B were written: a wave with b >= B did not return"
    return rc, ids[:B], nids[:B], st[:B], sc[:B]


_WORST = {}


def _record(route, rel):
    from tests.helpers import record_margin
    _WORST[route] = max(_WORST.get(route, 0.0), rel)
    record_margin("decoder_paths_%s_score_rel" % route, _WORST[route], SCORE_RTOL)


def check_beam(case, route, monkeypatch):
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    if route == "generic":
        monkeypatch.setenv("MDD_BEAM_GENERIC", "1")
    elif route in ("w2", "w3"):
        monkeypatch.setenv("MDD_BEAM_W", route[1])
    elif route != "auto":
        raise AssertionError(route)
    logp, lens, lm = inputs(case)
    want, wst, wsc = expected(case)
    rc, ids, nids, st, sc = gpu_beam(logp, lens, lm, case.beam, case.blank, case.alpha)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    assert (nids != SENT_I).all() and (st != SENT_I).all() and (sc != SENT_F).all(), "an output entry was not written"
    np.testing.assert_array_equal(st, wst, err_msg=case.name)
    np.testing.assert_array_equal(nids, [len(w) for w in want], err_msg=case.name)
    for b in range(case.B):
        assert ids[b, :nids[b]].tolist() == want[b], (case.name, route, b)
        assert (ids[b, nids[b]:] == SENT_I).all(), (case.name, route, b)        # nothing written past the winner
    ok = wst == 0
    assert np.isnan(sc[~ok]).all()
    rel = float(np.max(np.abs(sc[ok] - wsc[ok]) / np.abs(wsc[ok]))) if ok.any() else 0.0
    kernel = "generic" if route == "generic" or not fast_eligible(case.beam, case.C) else ("fast_packed" if case.B > 64 else "fast")
    print("%s [%s -> %s]: max relative score difference %.3e" % (case.name, route, kernel, rel))
    _record(kernel, rel)
    np.testing.assert_allclose(sc[ok], wsc[ok], rtol=SCORE_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,route", [(c.name, r) for c in CASES for r in c.routes])
def test_beam_paths_against_oracle(name, route, monkeypatch):
    check_beam(CASE_BY_NAME[name], route, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("beam,Cn", LIMIT_SHAPES)
def test_beam_T_limit(beam, Cn, monkeypatch):
    """The longest utterance the host accepts decodes like the oracle; one frame more is refused with MDD_ERR_ARG before any output
    is touched, and the library goes on working."""
    case = limit_case(beam, Cn)
    check_beam(case, "auto", monkeypatch)
    T = case.T + 1
    rs = np.random.Generator(np.random.PCG64(3))
    logp = _log_softmax(rs.standard_normal((T, 1, Cn)))
    lm = np.log(rs.uniform(0.01, 1.0, size=(Cn + 1, Cn + 1)))
    rc, ids, nids, st, sc = gpu_beam(logp, [T], lm, beam, 0, 0.0)
    assert rc == MDD_ERR_ARG
    msg = _L().mdd_last_error().decode()
    assert msg.startswith("mdd_beam") and "LDS" in msg, msg
    assert (ids == SENT_I).all() and (nids == SENT_I).all() and (st == SENT_I).all() and (sc == SENT_F).all()
    check_beam(CASE_BY_NAME["fast_flat_b16_C45_blank0"], "auto", monkeypatch)


# --------------------------------------------------------------------------------- mdd_diag_beam_stamps (the stamped instantiation)
STAMP_WORDS = 12
SENT_S = -(1 << 40)        # no cycle count and no list length is negative
STAMP_SHAPES = {"ns8": (5, 3), "ns16": (64, 16)}      # (C, beam): beam*C <= 512 is the 8-slot instantiation, 1024 the 16-slot one


def _stamp_case(Cn, beam):
    return Case("stamps_b%d_C%d" % (beam, Cn), "flat", Cn, beam, 0, 0.2, 12, 3, 900 + beam + Cn, lens=(12, 9, 5))


def gpu_beam_stamps(logp, lens, lm, beam, blank, alpha, null_stamps=False):
    """One mdd_diag_beam_stamps call on sentinel-filled outputs: (rc, ids, nids, status, score, stamps [B,12], guard [12]) as numpy.  The
    stamp buffer is the caller's own [B,12] words; the 12 words allocated behind it are the guard that must come back untouched."""
    T, B, Cn = logp.shape
    d_lp, d_len, d_lm = _dev(logp), _dev(np.asarray(lens, dtype=np.int32)), _dev(np.asarray(lm, dtype=np.float64))
    ids = torch.full((B, T), SENT_I, dtype=torch.int32, device="cuda")
    nids = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    st = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((B,), SENT_F, dtype=torch.float64, device="cuda")
    stamps = torch.full((B + 1, STAMP_WORDS), SENT_S, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_diag_beam_stamps(_ptr(d_lp), T, B, Cn, _ptr(d_len), beam, blank, _ptr(d_lm), C.c_double(alpha), _ptr(ids), _ptr(nids),
                                   _ptr(st), _ptr(sc), None if null_stamps else _ptr(stamps), None)
    torch.cuda.synchronize()
    stamps = stamps.cpu().numpy()
    return rc, ids.cpu().numpy(), nids.cpu().numpy(), st.cpu().numpy(), sc.cpu().numpy(), stamps[:B], stamps[B]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(STAMP_SHAPES))
def test_beam_stamps_entry_decodes_like_mdd_beam(shape, monkeypatch):
    """Both stamped instantiations: ids, nids, status and score are mdd_beam's on the same input, bit for bit; every word of stamps[B,12]
    was written, the eleven cycle sums are not negative; the 12 words behind the buffer are untouched."""
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    Cn, beam = STAMP_SHAPES[shape]
    case = _stamp_case(Cn, beam)
    assert fast_eligible(beam, Cn) and (beam * Cn <= 512) == (shape == "ns8")
    logp, lens, lm = inputs(case)
    rc0, ids0, nids0, st0, sc0 = gpu_beam(logp, lens, lm, beam, case.blank, case.alpha)
    assert rc0 == MDD_OK, _L().mdd_last_error().decode()
    rc, ids, nids, st, sc, stamps, guard = gpu_beam_stamps(logp, lens, lm, beam, case.blank, case.alpha)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    assert (nids0 != SENT_I).all() and (nids0 > 0).any(), "the input must decode"
    for name, a, b in (("ids", ids, ids0), ("nids", nids, nids0), ("status", st, st0), ("score", sc, sc0)):
        assert a.tobytes() == b.tobytes(), name
    print("%s: stamps of utterance 0: %s" % (case.name, stamps[0].tolist()))
    assert (stamps != SENT_S).all(), "a stamp word was not written"
    assert (stamps[:, :11] >= 0).all()
    assert (guard == SENT_S).all(), "words behind the stamp buffer were written"


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["generic_only_beam17", "null_stamps"])
def test_beam_stamps_entry_refuses_without_writing(why, monkeypatch):
    """A shape the plan does not send to the single-wave kernel, or no stamp buffer: MDD_ERR_ARG, nothing enqueued, every output's
    sentinels intact."""
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    Cn, beam = (5, 17) if why == "generic_only_beam17" else (5, 3)
    case = _stamp_case(Cn, beam)
    assert fast_eligible(beam, Cn) == (why == "null_stamps")
    logp, lens, lm = inputs(case)
    rc, ids, nids, st, sc, stamps, guard = gpu_beam_stamps(logp, lens, lm, beam, case.blank, case.alpha, null_stamps=why == "null_stamps")
    assert rc == MDD_ERR_ARG
    assert _L().mdd_last_error().decode().startswith("mdd_diag_beam_stamps"), _L().mdd_last_error().decode()
    assert (ids == SENT_I).all() and (nids == SENT_I).all() and (st == SENT_I).all() and (sc == SENT_F).all()
    assert (stamps == SENT_S).all() and (guard == SENT_S).all()


# ------------------------------------------------------------------------------------------------------------- greedy
GREEDY_SHAPES = ((2, 1, 1), (45, 63, 3), (45, 64, 3), (45, 65, 3), (64, 130, 2), (65, 130, 2), (200, 70, 2), (300, 20, 200))


@functools.lru_cache(maxsize=None)
def greedy_inputs(Cn, T, B):
    """Flat posteriors with tie rows patched in: exact values (0 is above every log-probability) so that both sides see equality."""
    rs = np.random.Generator(np.random.PCG64(700 + Cn + T + B))
    logp = _log_softmax(rs.standard_normal((T, B, Cn)))
    lens = rs.integers(1, T + 1, size=B).astype(np.int32)
    lens[0] = T
    if B > 1:
        lens[1] = T + 9
    if B > 2:
        lens[2] = 0
    if B > 3:
        lens[3] = 1
    rows = list(range(min(B, 2)))
    for b in rows:
        if T > 3:
            logp[2, b, :] = np.float32(-np.log(Cn))                      # an all-equal row: index 0
            logp[3, b, :] = -np.inf                                      # all -inf: torch.max gives index 0
        if T > 5 and Cn > 64:
            logp[4, b, [0, 64]] = 0.0                                    # the same lane in two strides: the earlier stride wins
            logp[5, b, [Cn - 65, Cn - 1]] = 0.0
        if T > 7 and Cn > 70:
            logp[6, b, [5, 70]] = 0.0                                    # lane 6 (second stride) against lane 5: class 5 wins
            logp[7, b, [70, 5]] = 0.0
        if T > 9 and Cn > 40:
            logp[8, b, [40, 7]] = 0.0                                    # two lanes of the same stride: the lower class wins
            logp[9, b, [33, 34, 35]] = 0.0
        for t in (63, 127):                                              # a repeat across a 64-frame group of the compaction
            if T > t + 1:
                k = 1 + (t + b) % (Cn - 1)
                logp[t, b, k] = 0.0
                logp[t + 1, b, k] = 0.0
        for t in (61, 125):                                              # and a kept pair right at the boundary
            if T > t + 1:
                logp[t, b, 1 + (t + b) % (Cn - 1)] = 0.0
    logp.setflags(write=False)
    lens.setflags(write=False)
    return logp, lens


def gpu_greedy(logp, lens, blank):
    T, B, Cn = logp.shape
    d_lp, d_len = _dev(logp), _dev(np.asarray(lens, dtype=np.int32))
    ids = torch.full((B, T), SENT_I, dtype=torch.int32, device="cuda")
    nids = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_greedy(_ptr(d_lp), T, B, Cn, _ptr(d_len), blank, _ptr(ids), _ptr(nids), None)
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), nids.cpu().numpy()


def check_greedy(logp, lens, blank):
    want = oracle.greedy(logp, lens, blank=blank)
    rc, ids, nids = gpu_greedy(logp, lens, blank)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    assert (nids != SENT_I).all()
    np.testing.assert_array_equal(nids, [len(w) for w in want])
    for b in range(logp.shape[1]):
        assert ids[b, :nids[b]].tolist() == want[b], b
        assert (ids[b, nids[b]:] == SENT_I).all(), b
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("blank_last", [False, True], ids=["blank0", "blankC-1"])
@pytest.mark.parametrize("Cn,T,B", GREEDY_SHAPES)
def test_greedy_paths_against_oracle(Cn, T, B, blank_last):
    logp, lens = greedy_inputs(Cn, T, B)
    check_greedy(logp, lens, Cn - 1 if blank_last else 0)


def test_greedy_tie_rows_decide_as_torch_max_does():
    """The patched rows of the greedy inputs mean what their comments say, on the oracle and on torch.max itself (CPU)."""
    logp, lens = greedy_inputs(200, 70, 2)
    am = torch.from_numpy(logp).argmax(-1).numpy()
    assert am[2:10, 0].tolist() == [0, 0, 0, 135, 5, 5, 7, 33]
    assert am[63, 0] == am[64, 0] != 0 and am[61, 0] != am[62, 0]
    for blank in (0, 199):
        want = oracle.greedy(logp, lens, blank=blank)
        for b in range(2):
            n, seq, prev = min(int(lens[b]), 70), [], None
            for t in range(n):
                k = int(am[t, b])
                if k != blank and not (t != 0 and k == prev):
                    seq.append(k)
                prev = k
            assert want[b] == seq


@pytest.mark.gpu
def test_greedy_T_limit():
    """T*4 bytes of dynamic LDS: the largest T the host accepts (150 KB) launches and decodes; blank runs and repeats span the groups."""
    T, Cn = GREEDY_MAX_T, 4
    rs = np.random.Generator(np.random.PCG64(9))
    z = rs.standard_normal((T, 1, Cn))
    z[np.arange(T) % 7 < 3] = z[0]                                       # runs of identical frames: repeats to collapse
    logp = _log_softmax(z)
    want = check_greedy(logp, np.array([T], dtype=np.int32), 0)
    assert 64 < len(want[0]) < T
    check_greedy(logp, np.array([T - 1], dtype=np.int32), Cn - 1)
