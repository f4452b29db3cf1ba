"""The f32x6 BiLSTM layer kernel writing the next projection's three bf16 planes itself (wave (1, 1) of every workgroup, while the owner
waves update cells) against the form it replaced (MDD_X6_OUT=fp32: fp32 layer outputs, then a split3_kernel pass): the same cell
arithmetic and the same split arithmetic, so the log-probs and every layer tap must agree bit for bit -- one, two, three and four row
tiles per team with ragged last tiles, H = 256, the raw-frame path, fused batches through graph replays, and the redo branch."""
import os
import subprocess

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pair(monkeypatch, geom, sd, taps=False):
    """(plane-writing model, fp32-output model) of the same weights; MDD_X6_OUT is read when a model is created."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    monkeypatch.delenv("MDD_X6_OUT", raising=False)
    new = HipModel(geom, sd, precision="f32x6", taps=taps)
    monkeypatch.setenv("MDD_X6_OUT", "fp32")
    old = HipModel(geom, sd, precision="f32x6", taps=taps)
    monkeypatch.delenv("MDD_X6_OUT")
    return new, old


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward_and_taps(m, x, x1, layers):
    out = m.forward(_cuda(x), _cuda(x1), sync_errors=True).clone()
    return out, [m.tap("rnn%d" % n).clone() for n in range(layers)]


# rows per team = ceil(B / 8), tiles of 16: B = 1, 3, 64 one tile (1 or 8 rows of it), 130 two (17 rows), 200 two (25), 300 three (38),
# 512 four (full)
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 38), (3, 122), (64, 500), (130, 60), (200, 100), (300, 60), (512, 500)])
def test_x6_plane_output_equals_fp32_output(B, T, monkeypatch):
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=83)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=7, seed=B + T, ragged=False)
    new, old = _pair(monkeypatch, geom, sd, taps=True)
    got, g_taps = _forward_and_taps(new, x, x1, geom.layers)
    want, w_taps = _forward_and_taps(old, x, x1, geom.layers)
    for n in range(geom.layers):
        assert g_taps[n].numel() == (T // 2) * B * 2 * geom.hidden
        assert torch.equal(_bits(g_taps[n]), _bits(w_taps[n])), "rnn%d" % n
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 128])
def test_x6_plane_output_equals_fp32_output_h256(B, monkeypatch):
    geom = synth.Geometry(**synth.REFERENCE_256)
    sd = synth.synth_state_dict(geom, seed=84)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=122, L=7, seed=B, ragged=False)
    new, old = _pair(monkeypatch, geom, sd, taps=True)
    got, g_taps = _forward_and_taps(new, x, x1, geom.layers)
    want, w_taps = _forward_and_taps(old, x, x1, geom.layers)
    for n in range(geom.layers):
        assert torch.equal(_bits(g_taps[n]), _bits(w_taps[n])), "rnn%d" % n
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_x6_plane_output_raw_equals_fp32_output(monkeypatch):
    B, T_raw = 64, 1001
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=5)
    raw = torch.from_numpy(synth.synth_raw_features(B, T_raw, 81, seed=T_raw)).cuda()
    _, x1, _, _ = synth.synth_batch(geom, B=B, T=T_raw // 2 * 2, L=5, seed=1, ragged=False)
    new, old = _pair(monkeypatch, geom, sd)
    got = new.forward_raw(raw, _cuda(x1), sync_errors=True)
    want = old.forward_raw(raw, _cuda(x1), sync_errors=True)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_x6_plane_output_fused_batches_equal_fp32_output(monkeypatch):
    """Batches of different padded lengths in one fused launch sequence, then three replays of the captured graph."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    shapes = [(5, 120, 9), (3, 64, 4), (7, 100, 12), (2, 120, 12), (4, 30, 1), (1, 2, 2)]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, T, L) in enumerate(shapes):
        x, x1, _, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=7 + 31 * k, ragged=True)
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    new, old = _pair(monkeypatch, geom, sd)
    args = (_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon))
    want = old.forward_fused(*args, sync_errors=True).cpu().numpy()
    for _ in range(4):   # the first call captures the graph, the next three replay it
        got = new.forward_fused(*args, sync_errors=True).cpu().numpy()
        for b in range(Bt):
            np.testing.assert_array_equal(got[:frames[b], b].view(np.int32), want[:frames[b], b].view(np.int32))


@pytest.mark.gpu
def test_x6_plane_output_redo_branch(monkeypatch):
    """MDD_X6_FORCE_REDO=4 declares every fourth phase stale: a redone tile's outputs are written once, from the redone sums."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=81)
    x, x1, _, _ = synth.synth_batch(geom, B=512, T=120, L=9, seed=512, ragged=True)
    new, old = _pair(monkeypatch, geom, sd)
    ref = new.forward(_cuda(x), _cuda(x1), sync_errors=True).clone()
    monkeypatch.setenv("MDD_X6_FORCE_REDO", "4")
    new_r, old_r = _pair(monkeypatch, geom, sd)
    got = new_r.forward(_cuda(x), _cuda(x1), sync_errors=True)
    want = old_r.forward(_cuda(x), _cuda(x1), sync_errors=True)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got), _bits(ref))


_PLAN_DRIVER = r'''
#include <iostream>
#include <sstream>
#include <string>
#include "plan.h"
using namespace mdd;
// stdin, one case per line: hidden mode B [SWITCH=value ...]  (other geometry: the reference's; every grid fits)
int main() {
    const char *env[] = {"MDD_PRECISION", "MDD_LSTM", "MDD_LSTM_X6", "MDD_X6_OUT"};
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        mdd_config c{243, 384, 4, 45, 32, 44, 512, 1e-5f};
        int mode, B;
        in >> c.hidden >> mode >> B;
        for (const char *e : env) unsetenv(e);
        for (std::string kv; in >> kv;) setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
        const Switches sw = read_switches();
        const ForwardPlan p = plan_forward(c, mode, sw, DeviceFit{true, true, true}, B);
        std::cout << p.planes_out << ' ' << sw.x6_out_fp32 << '\n';
    }
}
'''


def test_x6_plane_output_plan(tmp_path):
    """csrc/plan.h with the host compiler: the layer kernel writes the planes exactly where the f32x6 layer kernel feeds the f32x6 GEMM."""
    drv = tmp_path / "plan_driver.cpp"
    drv.write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc"),
                           str(drv), "-o", exe])
    cases = [("384 2 512", "1 0"), ("256 2 128", "1 0"), ("384 2 1", "1 0"), ("384 2 1024", "1 0"),
             ("384 2 512 MDD_X6_OUT=fp32", "0 1"), ("256 2 128 MDD_X6_OUT=fp32", "0 1"), ("384 2 512 MDD_X6_OUT=planes", "1 0"),
             ("384 2 512 MDD_LSTM_X6=0", "0 0"), ("384 2 512 MDD_LSTM=step", "0 0"), ("384 2 1025", "0 0"), ("256 2 129", "0 0"),
             ("384 0 512", "0 0"), ("384 1 512", "0 0"), ("256 0 128", "0 0"), ("256 1 128", "0 0")]
    r = subprocess.run([exe], input="\n".join(c for c, _ in cases) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.strip().split("\n")
    assert len(got) == len(cases)
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g, want)
