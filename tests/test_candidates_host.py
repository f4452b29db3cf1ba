"""The host side of the candidates feature, none of it needing a GPU: the dictionary's alternate pronunciations, the new ABI symbol in the
binding, the library and the header, and the GEMM launchers that do not run an operand period refusing one."""
import os
import re
import shutil
import subprocess

from tests.helpers import GOLD, ROOT

PKG = os.path.join(ROOT, "ctc-attention-mispronunciation_amd")


def test_cmu_dict_all_lists_every_pronunciation_in_dictionary_order():
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    p = Phonetic(os.path.join(GOLD, "cmudict_subset.dict"))
    assert p.cmu_dict_all("the") == ["DH AH0", "DH AH1", "DH IY0"]
    assert p.cmu_dict_all("The") == p.cmu_dict_all("the")
    assert p.cmu_dict_all("accept") == ["AE0 K S EH1 P T", "AH0 K S EH1 P T"]
    assert p.cmu_dict_all("about") == ["AH0 B AW1 T"]
    assert p.cmu_dict_all("zyzzyva") == []
    assert p.cmu_dict_all("accept(2)") == ["AH0 K S EH1 P T"]      # (an alternate's own key is a key like any other)
    # cmu_dict still answers the first entry alone
    assert p.cmu_dict("the") == "DH AH0" and p.cmu_dict("accept") == "AE0 K S EH1 P T" and p.cmu_dict("zyzzyva") is None
    assert p.api_word_phones_cmu(" about ") == "AH0 B AW1 T"
    for word in ("the", "accept", "about", "content", "thorough", "toronto", "read", "tomato"):
        assert p.cmu_dict_all(word)[0] == p.cmu_dict(word)


def test_forward_candidates_symbol_in_binding_library_and_header():
    from ctc_attention_mispronunciation_amd import _lib
    assert "mdd_forward_candidates" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "mdd_forward_candidates")
    with open(os.path.join(ROOT, "include", "mdd_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+mdd_forward_candidates\s*\(", header)
    for phrase in ("K,B,L", "plan_forward", "bit for bit"):
        assert phrase in header, phrase


_PERIOD_DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include "mdd_internal.h"
using namespace mdd;
// GemmOperand::period / SplitOperand::period are run by launch_gemm_nt and launch_gemm_bf16x3 alone.  Every other launcher must refuse a non-zero
// value with MDD_ERR_ARG before anything is launched or allocated: the pointers are never dereferenced.
int main() {
    static float a[64], w[64], c[64];
    static unsigned short h[64];
    const GemmOperand A{.p = a, .ld = 32}, W{.p = w, .ld = 32};
    const GemmOperand Ap{.p = a, .ld = 32, .period = 3}, Wp{.p = w, .ld = 32, .period = 3};
    const SplitOperand As{.p = {h, h}, .ld = 32}, Ws{.p = {h, h}, .ld = 32};
    const SplitOperand Asp{.p = {h, h}, .ld = 32, .stride = 0, .period = 3}, Wsp{.p = {h, h}, .ld = 32, .stride = 0, .period = 3};
    DeviceBuf xa, xb, part;
    int bad = 0;
    const auto refused = [&](const char *what, int rc) {
        const bool ok = rc == MDD_ERR_ARG && strstr(mdd_last_error(), "period") != nullptr;
        printf("%s: rc %d (%s)%s\n", what, rc, mdd_last_error(), ok ? "" : "  <-- not refused");
        bad += !ok;
    };
    refused("gemm_f32, A period", launch_gemm_f32(Ap, W, c, 32, 1, 1, 32, nullptr, {.batch = 6}));
    refused("gemm_f32, B period", launch_gemm_f32(A, Wp, c, 32, 1, 1, 32, nullptr, {.batch = 6}));
    refused("gemm_bf16x3_256, A period", launch_gemm_bf16x3_256(X3Form::Phase8, Asp, Ws, c, 32, 1, 1, 32, nullptr));
    refused("gemm_bf16x3_256, W period", launch_gemm_bf16x3_256(X3Form::SingleBarrier, As, Wsp, c, 32, 1, 1, 32, nullptr));
    refused("gemm_f32x6_ops, A period", gemm_f32x6_ops(Ap, W, nullptr, c, 32, 1, 1, 32, 1, xa, xb, part, nullptr));
    refused("gemm_f32x6_ops, B period", gemm_f32x6_ops(A, Wp, nullptr, c, 32, 1, 1, 32, 1, xa, xb, part, nullptr));
    refused("gemm_bf16x3_ops, A period", gemm_bf16x3_ops(Ap, W, nullptr, c, 32, 1, 1, 32, 1, xa, xb, part, nullptr));
    refused("gemm_bf16x3_ops, B period", gemm_bf16x3_ops(A, Wp, nullptr, c, 32, 1, 1, 32, 1, xa, xb, part, nullptr));
    // the two launchers that run a period refuse a negative one
    refused("gemm_nt, negative period", launch_gemm_nt({.p = a, .ld = 32, .period = -1}, W, c, 32, 1, 1, 32, nullptr, {.batch = 2}));
    refused("gemm_bf16x3, negative period", launch_gemm_bf16x3({.p = {h, h}, .ld = 32, .stride = 0, .period = -1}, Ws, c, nullptr, 32, 1, 1, 32, nullptr, {.batch = 2}));
    if (xa.p || xb.p || part.p) { printf("a refused call allocated\n"); bad++; }
    printf("%d not refused\n", bad);
    return bad != 0;
}
'''


def test_gemm_launchers_without_a_period_refuse_one(tmp_path):
    """A stand-alone program linked against the built library, in the manner of tests/test_host.py: every GEMM launcher that does not
    implement the operand period is called with period = 3 and must return MDD_ERR_ARG with a message that names it, before any launch (so no
    GPU is needed and the pointers are never dereferenced)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = str(tmp_path / "gemm_period.hip"), str(tmp_path / "gemm_period")
    with open(src, "w") as f:
        f.write(_PERIOD_DRIVER)
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), src, "-o", exe,
                           "-L", PKG, "-lmdd_hip", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 not refused" in r.stdout, r.stdout + r.stderr
