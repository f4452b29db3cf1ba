"""Diagnostic: per-phase cycle shares of beam_fast_kernel (mdd_diag_beam_stamps; the stamps go to a [B,12] buffer of their own)."""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, numpy as np
from ctc_attention_mispronunciation_amd import synth, _lib
from ctc_attention_mispronunciation_amd.utils.NgramLM import LanguageModel
T, B, Cn = 250, int(os.environ.get('B', '64')), 45
z = np.random.Generator(np.random.PCG64(1)).standard_normal((T, B, Cn)).astype(np.float32)
lp = torch.log_softmax(torch.from_numpy(z), -1).cuda()
lm = torch.from_numpy(LanguageModel(os.path.join(ROOT, 'tests/golden/lm_synth45.arpa')).dense_table(synth.phone_table_41(), Cn)).cuda()
lens = torch.full((B,), T, dtype=torch.int32, device='cuda')
ids = torch.empty((B, T), dtype=torch.int32, device='cuda'); nids = torch.empty(B, dtype=torch.int32, device='cuda'); st = torch.empty(B, dtype=torch.int32, device='cuda')
score = torch.zeros(B, dtype=torch.float64, device='cuda')
stamps = torch.zeros((B, 12), dtype=torch.int64, device='cuda')
for _ in range(2):
    _lib.check(_lib.lib().mdd_diag_beam_stamps(C.c_void_p(lp.data_ptr()), T, B, Cn, C.c_void_p(lens.data_ptr()), 10, 0, C.c_void_p(lm.data_ptr()), 0.0,
               C.c_void_p(ids.data_ptr()), C.c_void_p(nids.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(score.data_ptr()),
               C.c_void_p(stamps.data_ptr()), None))
torch.cuda.synchronize()
ph = stamps.cpu().numpy().astype(np.float64)
names = ['load/prefetch', 'candidates', 'copy+parent', 'verify', 'err', 'merge', 'lmax+lane-rank+theta', 'compact', 'rank', 'materialise', 'prefix copy', '(list len sum)']
tot = ph[:, :11].sum(1).mean()
for i, n in enumerate(names):
    print('%-22s %10.0f cycles/utt  %5.1f%%  (%.0f per frame)' % (n, ph[:, i].mean(), 100 * ph[:, i].mean() / tot, ph[:, i].mean() / T))
print('total stamped cycles/utt %.0f' % tot)
