"""Training steps WITH the optimizer on one handle, an eval-mode forward in between, held to float64 (GPU).  What the fixed-weight walk of
tests/test_train_walk.py cannot reach: updated weights feeding the next step's packed copies (launch_pack_gates, pack_w1, the split W_hh
planes), running statistics accumulating, Adam's step count and moments, the eval path picking up trained weights
(CTC_Model.mark_weights_changed) and the training handle surviving an eval pass.

Teacher-forced, so that fp32 and fp64 cannot drift apart and no new tolerance is needed: before each step the model's state_dict and the
optimizer's moments are read back, and the float64 reference of THIS step starts from those values.  Per step k (the shape changes every
step: train_walk_cases.TRAJECTORY; lr 1e-3, weight_decay 5e-4 as build_training sets):

1. oracle/ref_port.train_step(read-back state, batch k, masks k) in float64;
2. forward, CTCLoss(sum) / B, backward on the GPU;
3. log-probs, loss, gradients and the UPDATED running statistics (from the previous step's values, not the initial ones) at the bounds of
   tests/test_train_walk.py;
4. Adam.step(), then adam_f64 from the GPU's own (p, g, m, v): p', exp_avg, exp_avg_sq at the bounds of tests/test_adam.py;
   state['step'] == k for every parameter, num_batches_tracked advanced by k.

After steps 2 and 4: model.eval(), a no_grad forward of a batch of yet another shape against oracle/ref_port.forward(read-back state) in
float64 at 1e-4 (tests/test_geometry.py's bound for every precision), model.train(), and the trajectory goes on with the same train handle.
The read-back optim_dict of step 3 is loaded into a float64 torch.optim.Adam (load_state_dict), whose step 4 must be adam_f64's: the
interchange train.Adam's docstring promises, held to a reference.  Measured: profiles/train_walk_margins.json, "traj_*"."""
import copy

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import train_walk_cases as tw
from tests import test_adam as ta
from tests import test_train_walk as wk
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
LR, WD = 1e-3, 5e-4
EVAL_TOL = 1e-4
CASES = [("feat120_H64_L2_C20", "f32"), ("H256_L1", "f32"), ("H256_L1", "bf16x3")]


def _read_back(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_trajectory_teacher_forced(name, mode):
    from oracle import ref_port
    from ctc_attention_mispronunciation_amd.train import Adam
    torch.set_num_threads(min(16, torch.get_num_threads()))
    geom = tw.geometry(name)
    tol_m, tol_v = ta._bounds()
    bound = wk.bounds(name, mode)
    model = wk.make_model(geom, tw.state_dict(name))
    opt = Adam(model.parameters(), lr=LR, weight_decay=WD)
    names = [k for k, _ in model.named_parameters()]
    params = dict(model.named_parameters())
    handle, worst, resume = None, {}, None
    shapes = tw.TRAJECTORY[name]
    for k, shape in enumerate(shapes, start=1):
        tag = "traj_%s_%s step %d B%d T%d L%d" % ((name, mode, k) + shape)
        _, x, x1, masks, tg, il, tl = tw.inputs(name, shape)
        sd = _read_back(model)
        mom = {n: ((opt.state[params[n]]["exp_avg"].cpu().numpy(), opt.state[params[n]]["exp_avg_sq"].cpu().numpy()) if k > 1
                   else (np.zeros(params[n].shape, np.float32), np.zeros(params[n].shape, np.float32))) for n in names}
        ref = ref_port.train_step({n: v for n, v in sd.items() if "num_batches" not in n}, x, x1, masks, tg, il, tl, tw.P_DROP, dtype=torch.float64)
        got = wk.gpu_step(model, mode, (sd, x, x1, masks, tg, il, tl))
        if handle is None:
            handle = model._train_handle
        assert model._train_handle is handle and handle.handle, "one train handle for the whole trajectory"
        d = wk.distances(got, ref)
        wk.check_against_float64(tag, d, bound)
        for b_name, b_ in model.named_buffers():
            if b_name.endswith("num_batches_tracked"):          # (the synthetic state_dict starts its counters at 7)
                assert int(b_) == int(tw.state_dict(name)[b_name]) + k, (tag, b_name)
        # ---- the optimizer, from the GPU's own (p, g, m, v)
        if k == 4:                  # (a state_dict shares the optimizer's tensors, which the next step updates in place)
            resume = ({n: sd[n] for n in names}, {n: got[2][n] for n in names}, copy.deepcopy(opt.state_dict()))
        opt.step()
        torch.cuda.synchronize()
        e_p = e_m = e_v = 0.0
        for n in names:
            st = opt.state[params[n]]
            assert int(st["step"]) == k, (tag, n)
            g = got[2][n].astype(np.float32)
            rp, rm, rv = tw.adam_f64(sd[n], g, mom[n][0], mom[n][1], k, LR, wd=WD)
            gp, gm, gv = params[n].detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
            e_p = max(e_p, float((np.abs(gp - rp) / (2e-7 + 2e-6 * np.abs(rp))).max()))
            dm, dv = tw.adam_tensor_distances(gm, gv, rm, rv, sd[n], g, mom[n][0], mom[n][1], WD)
            e_m, e_v = max(e_m, dm), max(e_v, dv)
        print(tag, "| float64: logp %.2e loss %.2e grad %.2e conv %.2e running %.2e | adam: p %.3f of bound, exp_avg %.2e, exp_avg_sq %.2e"
              % (d["logp"], d["loss"], d["outside"], d["conv"], d["run"], e_p, e_m, e_v))
        for key, val in (("logp", d["logp"]), ("loss_rel", d["loss"]), ("grad_worst", d["outside"]), ("grad_conv_worst", d["conv"]), ("running_stats", d["run"]),
                         ("adam_param_of_bound", e_p), ("adam_exp_avg_of_scale", e_m), ("adam_exp_avg_sq_rel", e_v)):
            worst[key] = max(worst.get(key, 0.0), val)
        assert e_p <= 1 and e_m <= tol_m and e_v <= tol_v, (tag, e_p, e_m, e_v, tol_m, tol_v)
        # ---- an eval pass on the trained weights, then back to the same train handle
        if k in (2, 4):
            B, T, L = tw.EVAL_SHAPE
            xe, x1e = gc.draw_batch(geom, B, T, L, seed=900 + k)
            sd_now = _read_back(model)
            model.eval()
            with torch.no_grad():
                oute = model(wk._cuda(xe), wk._cuda(x1e)).cpu().numpy().astype(np.float64)
            model.train()
            refe = ref_port.forward({n: v for n, v in sd_now.items() if "num_batches" not in n}, xe, x1e, dtype=torch.float64).numpy()
            e_eval = float(np.abs(oute - refe).max())
            print(tag, "| eval forward on the trained weights: logp %.2e" % e_eval)
            worst["eval_logp"] = max(worst.get("eval_logp", 0.0), e_eval)
            assert e_eval <= EVAL_TOL, (tag, "eval", e_eval)
    handle.sync()
    tag = "traj_%s_%s" % (name, mode)
    budgets = dict(logp=bound[0], loss_rel=bound[1], grad_worst=bound[2], grad_conv_worst=wk.CONV_BOUND, running_stats=wk.RUN_BOUND,
                   adam_param_of_bound=1.0, adam_exp_avg_of_scale=tol_m, adam_exp_avg_sq_rel=tol_v, eval_logp=EVAL_TOL)
    for key, val in worst.items():
        record_margin("%s_%s" % (tag, key), val, budgets[key])
    # ---- resume: the optim_dict read back after step 3 in a float64 torch.optim.Adam; its step 4 is adam_f64's
    if resume is not None:
        p4, g4, osd = resume
        tparams = [torch.nn.Parameter(torch.tensor(p4[n], dtype=torch.float64)) for n in names]
        topt = torch.optim.Adam(tparams, lr=LR, weight_decay=WD)
        topt.load_state_dict({"state": {i: {kk: (vv.detach().cpu() if torch.is_tensor(vv) else vv) for kk, vv in s.items()} for i, s in osd["state"].items()},
                              "param_groups": osd["param_groups"]})
        for q, n in zip(tparams, names):
            q.grad = torch.tensor(g4[n].astype(np.float32), dtype=torch.float64)
        topt.step()
        for i, (q, n) in enumerate(zip(tparams, names)):
            st = topt.state[q]
            assert int(st["step"]) == 4 and st["exp_avg"].dtype == torch.float64
            m3, v3 = osd["state"][i]["exp_avg"].cpu().numpy(), osd["state"][i]["exp_avg_sq"].cpu().numpy()
            rp, rm, rv = tw.adam_f64(p4[n], g4[n].astype(np.float32), m3, v3, 4, LR, wd=WD)
            for a, b in ((q.detach().numpy(), rp), (st["exp_avg"].numpy(), rm), (st["exp_avg_sq"].numpy(), rv)):
                assert float(np.abs(a - b).max()) <= 1e-14 * max(float(np.abs(b).max()), tw.TINY), (name, n)
