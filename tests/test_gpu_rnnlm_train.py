"""GPU (-m gpu): training the recurrent LM (RecurrentLanguageModel.forward with a gradient wanted): the otr_lstm_* step kernels
against the numpy restatement tests/lstm_bptt_ref.py, and the whole model -- loss and every gradient -- against a CPU fp32 rebuild
from nn.Embedding + nn.LSTM + nn.Linear + the oracle's label-smoothing loss; FlatDataParallel + FusedAdam against torch's Adam;
dropout between the layers."""
import numpy as np
import pytest
import torch

from opentransformer_amd import _lib as L
from opentransformer_amd import ops
from opentransformer_amd import synthetic as syn
from opentransformer_amd.nn import PAD
from opentransformer_amd.recognize import LanguageModel
from oracle import otrans_oracle as orc
from tests import helpers as Hh
from tests import lstm_bptt_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.set_compute_dtype('bf16')
    ops._LSTM_FUSED = True


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_norm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def batch(B, T, V, seed, lengths=None):
    g = torch.Generator().manual_seed(seed)
    inp = torch.randint(1, V, (B, T), generator=g)
    tgt = torch.randint(1, V, (B, T), generator=g)
    lengths = lengths or [T - (3 * b) % max(T // 2, 1) for b in range(B)]
    for b, n in enumerate(lengths):
        inp[b, n:] = PAD
        tgt[b, n:] = PAD
    return inp, tgt


def cpu_rebuild(cfg, sd, inp, tgt, masks=None):
    """fp32 CPU: nn.Embedding -> nn.LSTM layer by layer (masks[k]: the dropout multiplier on layer k's output, [B, T, H]) -> tied
    nn.Linear -> the oracle's LabelSmoothingLoss.  -> (loss, {parameter name: gradient})"""
    V, Hd, nl = cfg['vocab_size'], cfg['hidden_size'], cfg['num_layers']
    emb = torch.nn.Embedding(V, Hd)
    emb.weight.data.copy_(sd['embedding.weight'])
    layers = []
    for k in range(nl):
        m = torch.nn.LSTM(Hd, Hd, batch_first=True)
        for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            getattr(m, n + '_l0').data.copy_(sd['rnn.%s_l%d' % (n, k)])
        layers.append(m)
    out = torch.nn.Linear(Hd, V)
    out.weight = emb.weight
    out.bias.data.copy_(sd['output_project.bias'])
    x = emb(inp)
    for k, m in enumerate(layers):
        if k and masks is not None:
            x = x * masks[k - 1]
        x = m(x)[0]
    loss = orc.label_smoothing_loss(out(x), tgt, cfg['smoothing'], PAD)
    loss.backward()
    g = {'embedding.weight': emb.weight.grad, 'output_project.bias': out.bias.grad}
    for k, m in enumerate(layers):
        for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            g['rnn.%s_l%d' % (n, k)] = getattr(m, n + '_l0').grad
    return loss.detach(), g


def device_lm(cfg, sd, mode):
    ops.set_compute_dtype(mode)
    lm = LanguageModel['rnn_lm'](cfg)
    lm.load_state_dict(sd)
    return lm.to(DEV).train()


def device_run(lm, inp, tgt, scale=None):
    lm.zero_grad(set_to_none=True)
    loss, aux = lm({'inputs': inp.to(DEV)}, {'targets': tgt.to(DEV)})
    assert aux is None
    (loss * scale if scale else loss).backward()
    torch.cuda.synchronize()
    g = {n: p.grad.detach().cpu() / (scale or 1.0) for n, p in lm.named_parameters()}
    return loss.detach().cpu(), g


SMALL = syn.rnn_lm_config(100, hidden_size=64, num_layers=2)


def test_fp32_training_matches_cpu_rebuild():
    """raised NotImplementedError before: forward with grad + backward in fp32 mode, B = 4, T = 13 with PAD tails"""
    sd = Hh.rnn_lm_state(SMALL)
    inp, tgt = batch(4, 13, 100, 1, lengths=[13, 9, 5, 11])
    want_loss, want = cpu_rebuild(SMALL, sd, inp, tgt)
    lm = device_lm(SMALL, sd, 'fp32')
    assert ops.lstm_fused_applies(4, 64)
    loss, got = device_run(lm, inp, tgt)
    assert abs(float(loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    assert sorted(got) == sorted(want)
    for n in want:
        assert rel(got[n], want[n]) <= 1e-4, (n, rel(got[n], want[n]))


def test_fp32_unfused_route_matches_cpu_rebuild():
    sd = Hh.rnn_lm_state(SMALL)
    inp, tgt = batch(4, 13, 100, 1, lengths=[13, 9, 5, 11])
    want_loss, want = cpu_rebuild(SMALL, sd, inp, tgt)
    lm = device_lm(SMALL, sd, 'fp32')
    ops._LSTM_FUSED = False
    loss, got = device_run(lm, inp, tgt)
    assert abs(float(loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    for n in want:
        assert rel(got[n], want[n]) <= 1e-4, (n, rel(got[n], want[n]))


# 16-bit modes: bound on max|loss error| relative, and on the relative norm of every gradient's error, against the fp32 rebuild;
# then the fused step kernels against the unfused route (same rounding points, different summation order)
@pytest.mark.parametrize('mode,tl,tg,tf', [('bf16', 1e-3, 1.5e-2, 1e-3), ('fp16', 2e-4, 2e-3, 2e-4)])
def test_16bit_training_matches_cpu_rebuild(mode, tl, tg, tf):
    sd = Hh.rnn_lm_state(SMALL)
    inp, tgt = batch(4, 13, 100, 1, lengths=[13, 9, 5, 11])
    want_loss, want = cpu_rebuild(SMALL, sd, inp, tgt)
    lm = device_lm(SMALL, sd, mode)
    scale = Hh.LOSS_SCALE if mode == 'fp16' else None
    loss, got = device_run(lm, inp, tgt, scale)
    errs = {n: rel_norm(got[n], want[n]) for n in want}
    print(mode, 'loss', abs(float(loss) / float(want_loss) - 1), 'grads', errs)
    assert abs(float(loss) - float(want_loss)) <= tl * abs(float(want_loss))
    for n in want:
        assert errs[n] <= tg, (n, errs[n])
    ops._LSTM_FUSED = False
    loss_u, got_u = device_run(lm, inp, tgt, scale)
    errs_u = {n: rel_norm(got[n], got_u[n]) for n in want}
    print(mode, 'fused vs unfused', abs(float(loss) - float(loss_u)), errs_u)
    assert abs(float(loss) - float(loss_u)) <= 1e-5 * abs(float(loss_u))
    for n in want:
        assert errs_u[n] <= tf, (n, errs_u[n])


# ---------------------------------------------------------------------------------------- the step kernels, one launch at a time
def _h16(mode):
    return {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[mode]


def _np(t):
    return t.detach().double().cpu().numpy()


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('B,Hd', [(1, 64), (13, 128), (16, 64), (64, 192), (4, 2048)])
@pytest.mark.parametrize('first', [True, False])
def test_step_kernels_against_restatement(mode, B, Hd, first):
    """otr_lstm_fwd_step (first: h_{t-1} = NULL, the zero state) and otr_lstm_bwd_step (first: dG_{t+1} = NULL, the last step)
    against lstm_bptt_ref's cell equations evaluated in float64 on the very operands the kernels read (16-bit-rounded h_{t-1},
    dG_{t+1} and W_hh in the 16-bit modes)"""
    ops.set_compute_dtype(mode)
    assert ops.lstm_fused_applies(B, Hd)
    cdt = _h16(mode)
    g = torch.Generator().manual_seed(B * 7 + Hd + int(first))
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
    w = rn(4 * Hd, Hd, sc=Hd ** -0.5)
    gx, bias = rn(B, 4 * Hd), rn(4 * Hd, sc=0.1)
    hp, cp = (None, None) if first else (rn(B, Hd, sc=0.5).to(cdt), rn(B, Hd))
    fwd, bwd = ops.lstm_pack_whh(w)
    h, c = torch.empty(B, Hd, device=DEV), torch.empty(B, Hd, device=DEV)
    h16 = torch.empty(B, Hd, device=DEV, dtype=cdt) if mode != 'fp32' else None
    act = torch.empty(B, 4 * Hd, device=DEV)
    lib, code, st = L.load(), ops._lstm_code(), ops._stream()
    p = ops._p
    L.check(lib.otr_lstm_fwd_step(p(gx), p(bias), p(hp), p(cp), p(fwd), p(h), p(h16), p(c), p(act), code, B, Hd, st), 'fwd_step')
    wr = _np(w.to(cdt))
    z = _np(gx) + _np(bias) + (0 if first else _np(hp) @ wr.T)
    a_r, c_r, h_r = ref.cell_fwd(z, None if first else _np(cp))
    tol = 2e-5
    assert np.abs(_np(act) - a_r).max() <= tol and np.abs(_np(c) - c_r).max() <= tol * max(1, np.abs(c_r).max())
    assert np.abs(_np(h) - h_r).max() <= tol
    if h16 is not None:
        assert torch.equal(h16, h.to(cdt))
    # backward step on the saved act / c
    dy = rn(B, Hd)
    dgn = None if first else rn(B, 4 * Hd, sc=0.3).to(cdt)
    dcin = None if first else rn(B, Hd)
    dcout = torch.empty(B, Hd, device=DEV)
    dg = torch.empty(B, 4 * Hd, device=DEV, dtype=cdt)
    L.check(lib.otr_lstm_bwd_step(p(dy), p(dgn), p(bwd), p(act), p(c), p(cp), p(dcin), p(dcout), p(dg), code, B, Hd, st), 'bwd_step')
    dh = _np(dy) + (0 if first else _np(dgn) @ wr)
    dg_r, dc_r = ref.cell_bwd(dh, None if first else _np(dcin), _np(act), _np(c), None if first else _np(cp))
    tdg = {'fp32': 2e-5, 'bf16': 8e-3, 'fp16': 1e-3}[mode]        # dG leaves in the compute type: one rounding
    assert np.abs(_np(dg) - dg_r).max() <= tdg * np.abs(dg_r).max(), np.abs(_np(dg) - dg_r).max()
    assert np.abs(_np(dcout) - dc_r).max() <= 2e-5 * max(1, np.abs(dc_r).max())


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,Hd', [(65, 64), (3, 96)])
def test_outside_the_limits_takes_the_unfused_route(mode, B, Hd):
    """a batch one past OTR_LSTM_MAX_ROWS, a width not a multiple of OTR_LSTM_HIDDEN_MULT: the step kernels refuse them, the layer
    takes the unfused route and is still right (one layer through ops.lstm_layer against the float64 restatement)"""
    ops.set_compute_dtype(mode)
    assert not ops.lstm_fused_applies(B, Hd)
    T = 5
    g = torch.Generator().manual_seed(B + Hd)
    wi, wh = torch.randn(4 * Hd, Hd, generator=g) * Hd ** -0.5, torch.randn(4 * Hd, Hd, generator=g) * Hd ** -0.5
    bi, bh = torch.randn(4 * Hd, generator=g) * 0.1, torch.randn(4 * Hd, generator=g) * 0.1
    x, dy = torch.randn(T, B, Hd, generator=g), torch.randn(T, B, Hd, generator=g)
    ps = [torch.nn.Parameter(t.to(DEV)) for t in (wi, wh, bi, bh)]
    xd = x.to(DEV).requires_grad_(True)
    h = ops.lstm_layer(xd, *ps)
    h.backward(dy.to(DEV))
    h_r, s = ref.layer_fwd(_np(x), _np(wi), _np(wh), _np(bi), _np(bh))
    dx_r, dwi_r, dwh_r, db_r, _ = ref.layer_bwd(_np(dy), _np(x), h_r, s, _np(wi), _np(wh))
    t = 1e-5 if mode == 'fp32' else 3e-2
    for got, want in ((h, h_r), (xd.grad, dx_r), (ps[0].grad, dwi_r), (ps[1].grad, dwh_r), (ps[2].grad, db_r), (ps[3].grad, db_r)):
        assert rel_norm(got, torch.from_numpy(want)) <= t


def test_yaml_size_bf16():
    """egs/aishell/conf/rnnlm.yaml's model (V 4233, H 1024, 2 layers, tied), B 16, T 40, dropout off, bf16 against the fp32 rebuild"""
    cfg = dict(syn.rnn_lm_yaml_config(), dropout=0.0)
    sd = Hh.rnn_lm_state(cfg)
    inp, tgt = batch(16, 40, 4233, 5)
    want_loss, want = cpu_rebuild(cfg, sd, inp, tgt)
    lm = device_lm(cfg, sd, 'bf16')
    assert ops.lstm_fused_applies(16, 1024)
    loss, got = device_run(lm, inp, tgt)
    errs = {n: rel_norm(got[n], want[n]) for n in want}
    print('yaml bf16 loss', abs(float(loss) / float(want_loss) - 1), 'grads', errs)
    assert abs(float(loss) - float(want_loss)) <= 1e-3 * abs(float(want_loss))
    for n in want:
        assert errs[n] <= 1.5e-2, (n, errs[n])


def test_flat_data_parallel_fused_adam_matches_torch_adam():
    """three FlatDataParallel + FusedAdam steps (the yaml's Adam settings, clip 5) in fp32 against torch.optim.Adam on the CPU
    rebuild's gradients; then the loss on a fixed batch goes down"""
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    o = syn.RNN_LM_YAML_OPTIM
    sd = Hh.rnn_lm_state(SMALL)
    inp, tgt = batch(4, 13, 100, 2)
    lm = device_lm(SMALL, sd, 'fp32')
    dp = FlatDataParallel(lm)
    opt = FusedAdam(dp, lr=o['lr'], betas=o['betas'], eps=o['eps'], weight_decay=o['weight_decay'], clip_grad=o['clip_grad'])
    ref_sd = {k: v.clone() for k, v in sd.items()}
    ref_sd['output_project.weight'] = ref_sd['embedding.weight']
    cpu_params = {k: torch.nn.Parameter(v) for k, v in ref_sd.items() if k != 'output_project.weight'}
    adam = torch.optim.Adam(list(cpu_params.values()), lr=o['lr'], betas=o['betas'], eps=o['eps'], weight_decay=o['weight_decay'])
    losses = []
    for step in range(3):
        dp.zero_grad()
        loss, _ = dp({'inputs': inp.to(DEV)}, {'targets': tgt.to(DEV)})
        ops.backward(loss)
        scale, _ = dp.all_reduce_gradients()
        opt.step(scale)
        lr = opt.stats()['lr']
        cur = {k: v.detach() for k, v in cpu_params.items()}
        cur['output_project.weight'] = cur['embedding.weight']
        want_loss, g = cpu_rebuild(SMALL, cur, inp, tgt)
        assert abs(loss.item() - float(want_loss)) <= 2e-5 * abs(float(want_loss)), (step, loss.item(), float(want_loss))
        for k, p in cpu_params.items():
            p.grad = g[k].clone()
        torch.nn.utils.clip_grad_norm_(list(cpu_params.values()), o['clip_grad'])
        for grp in adam.param_groups:
            grp['lr'] = lr
        adam.step()
        losses.append(loss.item())
        for n, p in lm.named_parameters():
            assert rel(p, cpu_params[n]) <= 1e-4, (step, n, rel(p, cpu_params[n]))
    for _ in range(5):
        dp.zero_grad()
        loss, _ = dp({'inputs': inp.to(DEV)}, {'targets': tgt.to(DEV)})
        ops.backward(loss)
        scale, _ = dp.all_reduce_gradients()
        opt.step(scale)
        losses.append(loss.item())
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0] - 0.02, losses


def _reseed(v=0x1234):
    ops.rng_seed_tensor(DEV).fill_(v)
    ops._state['rng_offset'] = 0


def test_dropout_between_layers(monkeypatch):
    """p > 0: the dropout acts on layer 0's output only (one call, on a [T, B, H] tensor), the same seed gives the same loss and
    gradients, eval() gives the p = 0 result, and the gradients match the rebuild with the device's mask"""
    cfg = syn.rnn_lm_config(100, hidden_size=64, num_layers=2, dropout=0.3)
    sd = Hh.rnn_lm_state(cfg)
    inp, tgt = batch(4, 13, 100, 3)
    lm = device_lm(cfg, sd, 'fp32')
    seen = []
    orig = ops.dropout

    def spy(x, p, training=True):
        y = orig(x, p, training)
        seen.append((x.detach().clone(), y.detach().clone(), p, training))
        return y
    monkeypatch.setattr(ops, 'dropout', spy)
    _reseed()
    loss1, g1 = device_run(lm, inp, tgt)
    assert len(seen) == 1 and seen[0][2] == 0.3 and seen[0][3] and tuple(seen[0][0].shape) == (13, 4, 64)
    x, y = seen[0][0], seen[0][1]
    keep = (y != 0)
    assert 0.6 < keep.float().mean().item() < 0.8
    assert torch.allclose(y[keep], x[keep] / 0.7, rtol=1e-6)
    _reseed()
    loss2, g2 = device_run(lm, inp, tgt)
    assert torch.equal(loss1, loss2)
    for n in g1:
        assert rel(g2[n], g1[n]) <= 1e-6, n      # atomic embedding scatter: the same sum, maybe in another order
    mask = (keep.float() / 0.7).permute(1, 0, 2).cpu()
    want_loss, want = cpu_rebuild(cfg, sd, inp, tgt, masks=[mask])
    assert abs(float(loss1) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    for n in want:
        assert rel(g1[n], want[n]) <= 1e-4, (n, rel(g1[n], want[n]))
    lm.eval()
    loss_e, g_e = device_run(lm, inp, tgt)
    loss_0, g_0 = cpu_rebuild(cfg, sd, inp, tgt)
    assert abs(float(loss_e) - float(loss_0)) <= 1e-5 * abs(float(loss_0))
    for n in g_0:
        assert rel(g_e[n], g_0[n]) <= 1e-4, n


def test_no_grad_forward_is_the_inference_path():
    """under torch.no_grad() forward keeps the decode path (no step kernels), and it agrees with the training path's loss"""
    sd = Hh.rnn_lm_state(SMALL)
    inp, tgt = batch(4, 13, 100, 4)
    lm = device_lm(SMALL, sd, 'fp32')
    with torch.no_grad():
        l0, _ = lm({'inputs': inp.to(DEV)}, {'targets': tgt.to(DEV)})
    l1, _ = lm({'inputs': inp.to(DEV)}, {'targets': tgt.to(DEV)})
    assert l1.requires_grad and not l0.requires_grad
    assert abs(l0.item() - l1.item()) <= 1e-5 * abs(l0.item())
