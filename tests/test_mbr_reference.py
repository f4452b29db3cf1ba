"""The MBR yardstick (tests/mbr_reference.py) and the host side of mdd_nbest_mbr, without a GPU.

  * the two symbols are declared, listed and exported;
  * the yardstick's distance is mdd_align's `dist` through the library on random pairs, and its batched numpy form is the same function;
  * every refusal of the entry: MDD_ERR_ARG before any device work, the message starting with the entry's name and naming the argument,
    and mdd_nbest_mbr_workspace_bytes 0 for every shape outside the ranges;
  * csrc/plan.h's mbr_plan and csrc/mbr.h's mbr_distance with the host compiler: the LDS the plan asks for fits a CU for every (C, words),
    its counts are the expressions written out, and the bit-vector recurrence -- the very function the kernel runs -- gives the plain DP's
    distance in every instantiation, at the word boundaries and on random pairs;
  * the yardstick's own rules (flags, ties) on hand-made lists;
  * infer --mbr: parsing, the refusals, and mbr_line's format.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mbr_reference as mr
from tests.helpers import GOLD, ROOT

CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")
MDD_ERR_ARG = -1
_FAKE = 4096      # a non-NULL value for pointers that must never be dereferenced: every call below is refused on the host


def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    assert re.search(r"\bint mdd_nbest_mbr\s*\(", header) and re.search(r"\bint64_t mdd_nbest_mbr_workspace_bytes\s*\(", header)
    for name in ("mdd_nbest_mbr", "mdd_nbest_mbr_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().mdd_version() == 100


# --------------------------------------------------------------------------------------------------------------- the distance
@pytest.mark.parametrize("alphabet", [2, 45])
def test_reference_distance_is_mdd_align_s(alphabet):
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import align_ids
    rs = np.random.default_rng(100 + alphabet)
    for trial in range(200):
        a = rs.integers(0, alphabet, size=int(rs.integers(1, 71))).tolist()
        b = mr.edited(rs, a, alphabet, 70, int(rs.integers(0, 6))) if trial % 2 else rs.integers(0, alphabet, size=int(rs.integers(1, 71))).tolist()
        if not b:
            b = [0]
        assert mr.distance(a, b) == align_ids((a, b))[0], (a, b)


def test_distance_with_an_empty_side_and_known_pairs():
    assert mr.distance([], []) == 0 and mr.distance([], [3, 4]) == 2 and mr.distance([5], []) == 1
    assert mr.distance("kitten", "sitting") == 3 and mr.distance("abc", "abc") == 0 and mr.distance("ab", "ba") == 2


def test_batched_distance_is_the_two_row_dp():
    rs = np.random.default_rng(7)
    for alphabet, width in ((2, 9), (45, 70), (256, 33)):
        n, m = 13, 11
        P, T = rs.integers(0, alphabet, size=(n, width)), rs.integers(0, alphabet, size=(m, width))
        plen, tlen = rs.integers(0, width + 1, size=n), rs.integers(0, width + 1, size=m)
        plen[:2], tlen[:2] = (0, width), (width, 0)
        got = mr.pair_distances(P, plen, T, tlen)
        for x in range(n):
            for y in range(m):
                assert got[x, y] == mr.distance(P[x, :plen[x]].tolist(), T[y, :tlen[y]].tolist()), (alphabet, x, y)


# ----------------------------------------------------------------------------------------------------------------- refusals
def _mbr_args(**over):
    a = dict(ids=_FAKE, pitch=64, nids=_FAKE, status=_FAKE, weight=_FAKE, N=10, B=2, C=45, max_len=64, ref=None, ref_len=None, ref_pitch=0,
             best=_FAKE, risk=_FAKE, dist=None, ref_dist=None, ref_risk=None, flag=_FAKE, ws=None, ws_bytes=0)
    a.update(over)
    vp = C.c_void_p
    return (vp(a["ids"]), a["pitch"], vp(a["nids"]), vp(a["status"]), vp(a["weight"]), a["N"], a["B"], a["C"], a["max_len"], vp(a["ref"]),
            vp(a["ref_len"]), a["ref_pitch"], vp(a["best"]), vp(a["risk"]), vp(a["dist"]), vp(a["ref_dist"]), vp(a["ref_risk"]), vp(a["flag"]),
            vp(a["ws"]), a["ws_bytes"], None)


_REFUSALS = [
    (dict(N=0), "N<=256"), (dict(N=257), "N<=256"), (dict(B=0), "B < 1"), (dict(C=1), "C<=256"), (dict(C=257), "C<=256"),
    (dict(max_len=0), "max_len"), (dict(max_len=1025, pitch=2000), "max_len"), (dict(max_len=65, pitch=64), "max_len"),
    (dict(ids=None), "ids_dev"), (dict(nids=None), "nids_dev"), (dict(weight=None), "weight_dev"), (dict(best=None), "best_dev"),
    (dict(risk=None), "risk_dev"), (dict(flag=None), "flag_dev"),
    (dict(ref_dist=_FAKE), "ref_dist_dev"), (dict(ref_risk=_FAKE), "ref_risk_dev"),
    (dict(ref=_FAKE, ref_pitch=8), "ref_len_dev"), (dict(ref_len=_FAKE, ref_pitch=8), "ref_dev"),
    (dict(ref=_FAKE, ref_len=_FAKE, ref_pitch=0), "ref_pitch"),
]


@pytest.mark.parametrize("over,needle", _REFUSALS, ids=["_".join("%s=%s" % kv for kv in o.items()) for o, _ in _REFUSALS])
def test_bad_arguments_are_refused_on_the_host(over, needle):
    """Refused before any device call (this runs without a GPU); a shape outside the ranges has no workspace size."""
    L = _L()
    assert L.mdd_nbest_mbr(*_mbr_args(**over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_nbest_mbr") and needle in msg, msg
    if set(over) & {"N", "B", "C"} or over.get("max_len") in (0, 1025):
        a = dict(N=10, B=2, C=45, max_len=64)
        a.update({k: v for k, v in over.items() if k in a})
        assert L.mdd_nbest_mbr_workspace_bytes(a["N"], a["B"], a["C"], a["max_len"]) == 0


def test_status_dev_is_optional_and_a_short_workspace_is_refused():
    L = _L()
    need = L.mdd_nbest_mbr_workspace_bytes(10, 2, 45, 64)
    assert need == 2 * 16 * 16 * 4                                      # B x (64 ids / 4) words x (N + 1 -> 16) columns x 4 bytes
    assert L.mdd_nbest_mbr_workspace_bytes(256, 3, 256, 1024) == 3 * 256 * 272 * 4
    assert L.mdd_nbest_mbr(*_mbr_args(ws=_FAKE, ws_bytes=need - 1)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_nbest_mbr") and "workspace_bytes %d, need %d" % (need - 1, need) in msg, msg


# ------------------------------------------------------------------------------------------- plan.h and mbr.h on the host
_DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mbr.h"
using namespace mdd;

static long bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)((rng_state >> 11) % n); }

static int dp(const std::vector<int> &a, const std::vector<int> &b) {
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); j++) prev[j] = (int)j;
    for (size_t i = 1; i <= a.size(); i++) {
        cur[0] = (int)i;
        for (size_t j = 1; j <= b.size(); j++) {
            int v = prev[j - 1] + (a[i - 1] != b[j - 1]);
            if (prev[j] + 1 < v) v = prev[j] + 1;
            if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
            cur[j] = v;
        }
        prev.swap(cur);
    }
    return prev[b.size()];
}

// the kernel's data: the match table of the pattern, the packed text in a column of stride `stride`
template <int NW> static int bitvector(const std::vector<int> &p, const std::vector<int> &t, int C) {
    std::vector<unsigned long long> peq((size_t)C * NW, 0);
    for (size_t j = 0; j < p.size(); j++) peq[(size_t)p[j] * NW + j / 64] |= 1ull << (j % 64);
    const int stride = 5;
    std::vector<uint32_t> text(((size_t)64 * NW / 4) * stride, 0xffffffffu);       // the other columns and the tail: never read
    for (size_t j = 0; j < t.size(); j++) {
        uint32_t &w = text[(j / 4) * stride + 2];
        w = (w & ~(255u << (8 * (j % 4)))) | ((uint32_t)t[j] << (8 * (j % 4)));
    }
    return mbr_distance<NW>(peq.data(), text.data() + 2, stride, (int)p.size(), (int)t.size());
}

template <int NW> static long pairs_of(int C) {
    long n = 0;
    const int cap = 64 * NW;
    int edges[] = {1, 2, 63, 64, 65, 127, 128, 129, cap / 2, cap / 2 + 1, cap - 1, cap};
    std::vector<int> lens;
    for (int e : edges) if (e >= 1 && e <= cap) lens.push_back(e);
    for (int trial = 0; trial < 60 + 4 * (int)(lens.size() * lens.size()); trial++) {
        int lp, lt;
        const int ne = (int)lens.size();
        if (trial < 4 * ne * ne) { lp = lens[(trial / 4) % ne]; lt = lens[(trial / 4) / ne]; }
        else { lp = 1 + (int)rnd(cap); lt = (int)rnd(cap + 1); }
        std::vector<int> p(lp), t;
        for (int &v : p) v = (int)rnd(C);
        if (trial % 4 == 0) { t.resize(lt); for (int &v : t) v = (int)rnd(C); }
        else {                                   // a few edits of the pattern, as two hypotheses of one list differ
            t = p;
            for (int e = (int)rnd(6); e > 0; e--) {
                const unsigned op = rnd(3), at = rnd((unsigned)t.size() + 1);
                if (op == 0 && at < t.size()) t[at] = (int)rnd(C);
                else if (op == 1 && (int)t.size() < cap) t.insert(t.begin() + at, (int)rnd(C));
                else if (op == 2 && at < t.size()) t.erase(t.begin() + at);
            }
            if (trial % 4 == 1 && lt <= (int)t.size()) t.resize(lt);
        }
        if (trial % 16 == 3) p[rnd(lp)] = C - 1;
        const int want = dp(p, t), got = bitvector<NW>(p, t, C);
        CHECK(want == got, "NW %d C %d plen %d tlen %zu: bit-vector %d, DP %d", NW, C, lp, t.size(), got, want);
        n++;
    }
    return n;
}

int main() {
    // the plan: its counts written out, and the LDS of every (C, words) inside a CU
    size_t worst = 0;
    for (int C = 2; C <= 256; C++)
        for (int max_len = 1; max_len <= 1024; max_len++)
            for (int N : {1, 2, 15, 16, 63, 64, 65, 200, 255, 256}) {
                const MbrPlan p = mbr_plan(N, 3, C, max_len);
                int words = 1;
                while (64 * words < max_len) words *= 2;
                const int NP = (N + 1 + 15) / 16 * 16;
                CHECK(p.words == words && words <= 16 && p.Lp == 64 * words && p.NP == NP && NP > N, "C %d max_len %d N %d: words %d Lp %d NP %d", C, max_len, N, p.words, p.Lp, p.NP);
                CHECK(p.text_in_lds == (max_len <= 64), "C %d max_len %d: text_in_lds %d", C, max_len, p.text_in_lds);
                const size_t smem = (size_t)8 * 4 * C * words + (max_len <= 64 ? (size_t)4 * 16 * NP : 0);
                CHECK(p.smem == smem && p.smem <= 160 * 1024, "C %d max_len %d N %d: smem %zu, written out %zu", C, max_len, N, p.smem, smem);
                CHECK(p.utt == (size_t)4 * 16 * words * NP && p.bytes == 3 * p.utt, "C %d max_len %d N %d: utt %zu bytes %zu", C, max_len, N, p.utt, p.bytes);
                if (p.smem > worst) worst = p.smem;
            }
    CHECK(!mbr_shape_ok(0, 1, 45, 64) && !mbr_shape_ok(257, 1, 45, 64) && !mbr_shape_ok(1, 0, 45, 64) && !mbr_shape_ok(1, 1, 1, 64) &&
          !mbr_shape_ok(1, 1, 257, 64) && !mbr_shape_ok(1, 1, 45, 0) && !mbr_shape_ok(1, 1, 45, 1025) && mbr_shape_ok(256, 1, 256, 1024) &&
          mbr_shape_ok(1, 1, 2, 1), "mbr_shape_ok");
    printf("largest LDS of a workgroup: %zu bytes\n", worst);
    // the recurrence
    long n = 0;
    for (int C : {2, 45, 256}) {
        n += pairs_of<1>(C); n += pairs_of<2>(C); n += pairs_of<4>(C); n += pairs_of<8>(C); n += pairs_of<16>(C);
    }
    printf("%ld pairs; %ld mismatch(es)\n", n, bad);
    return bad != 0;
}
'''


def test_mbr_plan_and_the_bit_vector_distance_on_the_host(tmp_path):
    src, exe = tmp_path / "mbr_driver.cpp", str(tmp_path / "mbr_driver")
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "; 0 mismatch(es)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    assert int(re.search(r"largest LDS of a workgroup: (\d+) bytes", r.stdout).group(1)) == 128 * 1024      # C = 256, 16 words, four tables
    assert int(re.search(r"(\d+) pairs", r.stdout).group(1)) > 4000


# ------------------------------------------------------------------------------------------------- the yardstick's own rules
def _tiny(rows, weights, status=None, C=9, max_len=4, ref=None):
    N = len(rows)
    ids, nids = np.zeros((N, 1, 4), dtype=np.int32), np.zeros((N, 1), dtype=np.int32)
    for n, row in enumerate(rows):
        ids[n, 0, :len(row)], nids[n, 0] = row, len(row)
    kw = {}
    if ref is not None:
        kw = dict(ref=np.array([ref + [0] * (4 - len(ref))], dtype=np.int32), ref_len=np.array([len(ref)], dtype=np.int32))
    return mr.reference(ids, nids, status, np.array(weights, dtype=np.float64).reshape(N, 1), C, max_len, **kw)


def test_reference_rules_on_hand_made_lists():
    r = _tiny([[1, 2, 3], [1, 2], [1, 2, 4], [1, 2]], [0.25, 0.25, 0.25, 0.25], ref=[1, 2, 3])
    assert r["dist"][0].tolist() == [[0, 1, 1, 1], [1, 0, 1, 0], [1, 1, 0, 1], [1, 0, 1, 0]]
    assert r["risk"][:, 0].tolist() == [0.75, 0.5, 0.75, 0.5] and r["best"][0] == 1 and r["flag"][0] == 0      # the duplicate ties: the lower rank
    assert r["ref_dist"][:, 0].tolist() == [0, 1, 1, 1] and r["ref_risk"][0] == 0.75
    r = _tiny([[1, 2, 3], [1, 2], [1, 2, 4], [1, 2]], [0.5, 0.0, 0.5, 0.0])
    assert r["risk"][:, 0].tolist() == [0.5, 1.0, 0.5, 1.0] and r["best"][0] == 0
    r = _tiny([[1, 2], [3, 1, 2], [1, 2, 4], [1, 5, 2]], [0.0, 0.25, 0.25, 0.25])   # the zero-weight row has the least risk and is not chosen
    assert r["risk"][:, 0].tolist() == [0.75, 1.0, 1.0, 1.0] and r["best"][0] == 1
    r = _tiny([[1, 2, 3, 4], [1, 2], [2]], [0.0, 0.0, 1.0])                  # all weight on one rank
    assert r["best"][0] == 2 and r["risk"][:, 0].tolist() == [3.0, 1.0, 0.0]
    assert _tiny([[1], [2]], [0.0, 0.0])["flag"][0] == 1 and _tiny([[1], [2]], [1.0, 1.0], status=[3])["flag"][0] == 1
    for r in (_tiny([[1, 9], [2]], [1.0, 1.0]), _tiny([[1], [2]], [1.0, 1.0], ref=[-1]), _tiny([[1, 2, 3, 4], [2]], [1.0, 1.0], max_len=3),
              _tiny([[1, 9], [2]], [0.0, 0.0])):
        assert r["flag"][0] == 2 and r["best"][0] == -1 and np.isnan(r["risk"]).all() and (r["dist"] == -1).all()
    assert _tiny([[1, 9], [2]], [1.0, 1.0], status=[1])["flag"][0] == 1      # a skipped utterance is not looked at


# ------------------------------------------------------------------------------------------------------------- infer --mbr
def _conf(tmp_path, decode_type, beam_width=10):
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nright_ctx: 2\nn_skip_frame: 2\nbatch_size: 4\n"
                    "decode_type: '%s'\nbeam_width: %d\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "none", tmp_path / "none", decode_type, beam_width, os.path.join(GOLD, "lm_synth45.arpa")))
    return str(conf)


def test_parse_args_takes_mbr():
    from ctc_attention_mispronunciation_amd import infer
    assert infer.parse_args(["--conf", "c", "--wav_transcript_path", "d"]).mbr is None
    a = infer.parse_args(["--conf", "c", "--wav_transcript_path", "d", "--mbr", "5", "--nbest", "3"])
    assert (a.mbr, a.nbest) == (5, 3)
    with pytest.raises(SystemExit):
        infer.parse_args(["--conf", "c", "--wav_transcript_path", "d", "--mbr", "five"])


@pytest.mark.parametrize("decode_type,n,needle", [("Greedy", 3, "greedy"), ("Beam", 1, "at least 2"), ("Beam", 0, "at least 2"),
                                                  ("Beam", 11, "beam_width = 10")])
def test_main_refuses_mbr(tmp_path, capsys, decode_type, n, needle):
    """Refused through ``refuse`` (status 2, one line on stderr) as soon as the conf is read: before the model, the dictionary and the
    device are touched, and with nothing written into the input folder."""
    from ctc_attention_mispronunciation_amd import infer
    data = tmp_path / "words"
    data.mkdir()
    with pytest.raises(SystemExit) as e:
        infer.main(["--conf", _conf(tmp_path, decode_type), "--wav_transcript_path", str(data), "--mbr", str(n)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("--mbr") and needle in err and err.count("\n") == 1, err
    assert os.listdir(str(data)) == []


def test_infer_core_refuses_mbr_without_a_beam_decoder():
    from ctc_attention_mispronunciation_amd import infer_core

    class Greedy(object):
        pass

    class Beam(object):
        beam_width = 10
        decode_mbr = None

    for dec, n in ((Greedy(), 3), (Beam(), 1), (Beam(), 11)):
        with pytest.raises(ValueError, match="mbr needs"):
            infer_core.infer(None, {}, [], None, None, dec, None, {}, False, mbr=n)


def test_mbr_line_format():
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.infer_core import diagnose, mbr_line
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import Decoder
    dec = Decoder(synth.phone_table_41(), space_idx=-1, blank_index=0)
    canonical = "k ae t"
    d = diagnose("k ah t", canonical, dec)
    comp = "%d/%d" % (d["correct"], d["correct"] + d["del_sub"])
    assert comp == "2/3"
    assert mbr_line(("k ah t", 2, 0.25, 1.0 / 3, 1.5), canonical, dec) == "mbr    : 3 k ah t | risk 0.2500 | risk1 0.3333 | exp 1.5000 | Comp. 2/3"
    assert mbr_line(("k ae t", 0, 0.0, 0.0, None), canonical, dec) == "mbr    : 1 k ae t | risk 0.0000 | risk1 0.0000 | exp - | Comp. 3/3"
    assert mbr_line(None, canonical, dec) == "mbr    : -"
    assert mbr_line(("", 1, 2.0, 3.0, 3.0), canonical, dec) == "mbr    : 2  | risk 2.0000 | risk1 3.0000 | exp 3.0000 | Comp. -"
