"""CPU (-m "not gpu"): tests/lstm_bptt_ref.py -- the equations the otr_lstm_* kernels implement -- against torch autograd through
nn.LSTM, and the yaml-size recurrent-LM config."""
import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import lstm_bptt_ref as ref


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize('H,B,T,p', [(8, 3, 5, 0.0), (16, 1, 7, 0.0), (12, 4, 1, 0.0), (8, 5, 6, 0.5)])
def test_restatement_matches_torch_autograd(H, B, T, p):
    torch.manual_seed(H * 100 + B * 10 + T)
    lstm = torch.nn.LSTM(H, H, num_layers=2, batch_first=True, dropout=0.0).double()
    x = torch.randn(B, T, H, dtype=torch.float64, requires_grad=True)
    w = torch.randn(B, T, H, dtype=torch.float64)
    mask = None
    if p > 0:    # nn.LSTM's inter-layer dropout restated with an explicit mask on layer 0's output
        mask = (torch.rand(B, T, H) >= p).double() / (1 - p)
        l0 = torch.nn.LSTM(H, H, batch_first=True).double()
        l1 = torch.nn.LSTM(H, H, batch_first=True).double()
        for k, m in ((0, l0), (1, l1)):
            for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
                getattr(m, n + '_l0').data.copy_(getattr(lstm, '%s_l%d' % (n, k)).data)
        y = l1(l0(x)[0] * mask)[0]
        params = [(l0, 0), (l1, 0)]
    else:
        y = lstm(x)[0]
        params = [(lstm, 0), (lstm, 1)]
    loss = (y * w).sum()
    loss.backward()
    layers = [tuple(getattr(m, '%s_l%d' % (n, k)).detach().numpy() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
              for m, k in params]
    tm = lambda t: t.detach().numpy().transpose(1, 0, 2).copy()
    masks = [tm(mask)] if mask is not None else None
    h, dx, grads = ref.stack_fwd_bwd(tm(x), layers, tm(w), masks)
    assert _rel(h, tm(y)) < 1e-12
    assert _rel(dx, tm(x.grad)) < 1e-12
    for (m, k), (dwi, dwh, db) in zip(params, grads):
        assert _rel(dwi, getattr(m, 'weight_ih_l%d' % k).grad.numpy()) < 1e-12
        assert _rel(dwh, getattr(m, 'weight_hh_l%d' % k).grad.numpy()) < 1e-12
        assert _rel(db, getattr(m, 'bias_ih_l%d' % k).grad.numpy()) < 1e-12
        assert _rel(db, getattr(m, 'bias_hh_l%d' % k).grad.numpy()) < 1e-12     # the two biases get identical gradients


def test_step_form_matches_sequence_form():
    """layer_bwd's step loop gives the dG that the unrolled product of every step's cell Jacobian gives: checked by finite
    differences of one weight of W_hh"""
    rng = np.random.default_rng(3)
    H, B, T = 4, 2, 4
    wi, wh = rng.standard_normal((4 * H, H)) * 0.5, rng.standard_normal((4 * H, H)) * 0.5
    bi, bh = rng.standard_normal(4 * H) * 0.1, rng.standard_normal(4 * H) * 0.1
    x, dy = rng.standard_normal((T, B, H)), rng.standard_normal((T, B, H))
    h, s = ref.layer_fwd(x, wi, wh, bi, bh)
    _, _, dwh, _, _ = ref.layer_bwd(dy, x, h, s, wi, wh)
    eps = 1e-6
    for (r, q) in ((0, 1), (5, 2), (13, 3)):
        wp, wm = wh.copy(), wh.copy()
        wp[r, q] += eps
        wm[r, q] -= eps
        num = ((ref.layer_fwd(x, wi, wp, bi, bh)[0] - ref.layer_fwd(x, wi, wm, bi, bh)[0]) * dy).sum() / (2 * eps)
        assert abs(num - dwh[r, q]) < 1e-7 * max(1.0, abs(num))


def test_rnn_lm_yaml_config():
    cfg = syn.rnn_lm_yaml_config()
    assert (cfg['vocab_size'], cfg['num_layers'], cfg['hidden_size'], cfg['dropout'], cfg['share_embedding'], cfg['smoothing']) == \
        (4233, 2, 1024, 0.1, True, 0.1)
    assert syn.RNN_LM_YAML_OPTIM == dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-6, clip_grad=5.0, batch_size=16)
