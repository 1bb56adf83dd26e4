"""GPU (-m gpu): minimum word error rate training of the CTC model.  otr_ctc_mwer_loss against the numpy float64 restatement
(tests/ctc_mwer_ref.py) on the cases of tests/ctc_mwer_cases.py, its structural promises (every cell of the gradient written, exact
zeros, the same scalars on every run and without a gradient), and CTCMWERTraining against the loss composed from torch ops.

Tolerances: seq_logp 1e-4 + 1e-6 |s| and post / utt_err / loss 4 eps max(1, W_max), as tests/test_gpu_mwer.py; dlogits within
max(1e-6 g, 4 d0) of the restatement, d0 the float32 floor of the case: the largest distance between the torch composition run in
float32 and in float64 on the same inputs on the CPU.  Every kernel case appends (error, d0, ratio) to
parity_out/ctc_mwer_tolerance.jsonl (or under $OTR_PARITY_DIR) before it asserts."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import ctc_loss_cases as cc
from tests import ctc_mwer_cases as cases
from tests import ctc_mwer_ref as ref
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {'noref': (False, 0.0, 1.0), 'w0_s0.1': (True, 0.0, 0.1), 'w0.3': (True, 0.3, 1.0), 'w0.3_s0.1': (True, 0.3, 0.1)}


def _record(rec):
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'ctc_mwer_tolerance.jsonl'), 'a') as f:
        f.write(json.dumps({k: (float('%.4g' % v) if isinstance(v, float) else v) for k, v in rec.items()}, sort_keys=True) + '\n')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(kind, V=0, N=0):
    """(case with float32-representable logits, dead [B, N]) -- built once, never changed"""
    if kind == 'big':
        c, dead = cases.big_case()
    else:
        T = 39 if kind == 'odd' else 40                     # T * V odd: utterances 1.. start off a 16-byte boundary, chunks end mid-quad
        main = cases.main_case(1000 * N + V + T, 4, T, V, N)
        c, dead = cases.with_edges(main, V)
    c['logits'] = c['logits'].astype(np.float32).astype(np.float64)
    return c, dead


@functools.lru_cache(maxsize=None)
def _want(kind, V, N, mode):
    """the restatement's outputs and gradient and the float32 floor d0 of the gradient, computed once per case and mode"""
    c, dead = _case(kind, V, N)
    with_ref, w, scale = MODES[mode]
    a = (c['logits'], c['in_len'], c['hyps'], c['hyp_len'], c['errors']) + ((c['ref'], c['ref_len']) if with_ref else (None, None))
    f = ref.forward(*a, ctc_weight=w, scale=scale)
    assert np.array_equal(f['live'], ~dead)
    f['grad'] = ref.grad(*a, ctc_weight=w, scale=scale)
    d64 = cases.compose_torch(c, f['live'], w, scale, with_ref, torch.float64)[3]
    d32 = cases.compose_torch(c, f['live'], w, scale, with_ref, torch.float32)[3]
    assert np.abs(f['grad'] - d64).max() < 1e-8
    f['d0'] = float(np.abs(d32.astype(np.float64) - d64).max())
    return f


def _run(c, mode, grad=True, offset=0, gscale=None, errors=None, ctc_weight=None):
    """otr_ctc_mwer_loss through the library's own entry on ops.log_softmax of the logits; every output starts as NaN, the gradient
    too (offset: its base that many floats behind an aligned address).  Returns the outputs as numpy arrays."""
    from opentransformer_amd import _lib, ops
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    with_ref, w, scale = MODES[mode]
    w = w if ctc_weight is None else ctc_weight
    B, T, V = c['logits'].shape
    N, W = c['hyps'].shape[1:]
    lp = ops.log_softmax(_dev(c['logits'].astype(np.float32)))
    il, hy, hl = _dev(c['in_len'].astype(np.int32)), _dev(c['hyps']), _dev(c['hyp_len'].astype(np.int32))
    er = _dev((c['errors'] if errors is None else errors).astype(np.int32))
    rf, rl = (_dev(c['ref']), _dev(c['ref_len'].astype(np.int32))) if with_ref else (None, None)
    max_tgt = min(max(W, c['ref'].shape[1] if with_ref else 0), 127)
    assert W >= max_tgt and (not with_ref or c['ref'].shape[1] >= max_tgt)
    nan = lambda *sh: torch.full(sh, float('nan'), device=DEV)              # noqa: E731
    out = {'loss3': nan(3), 'seq_logp': nan(B, N), 'post': nan(B, N), 'utt_err': nan(B), 'nll_ref': nan(B)}
    buf = nan(B * T * V + offset) if grad else None
    dl = buf[offset:] if grad else None
    nws = lib.otr_ctc_mwer_workspace_floats(B, N, T, max_tgt)
    assert nws == (N + 1) * B * T * (2 * max_tgt + 1) + B * (N + 1)
    ws = nan(nws)
    rc = lib.otr_ctc_mwer_loss(p(lp), p(il), p(hy), W, p(hl), p(er), p(rf), c['ref'].shape[1] if with_ref else 0, p(rl), w, scale, p(gscale),
                               B, N, T, V, max_tgt, cases.BLANK, p(out['loss3']), p(out['seq_logp']), p(out['post']), p(out['utt_err']),
                               p(out['nll_ref']), p(dl), p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.otr_last_error_string()
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['dlogits'] = dl.cpu().numpy().reshape(B, T, V) if grad else None
    res['lp'] = lp
    return res


SCALARS = ('loss3', 'seq_logp', 'post', 'utt_err', 'nll_ref')


def _check(tag, c, got, want, g=1.0):
    live = want['live']
    s_want = want['seq_logp']
    eps = 1e-4 + 1e-6 * np.abs(s_want[live]).max() if live.any() else 1e-4
    w_max = max(1, int(c['errors'].max()))
    assert np.array_equal(got['seq_logp'] == -np.inf, ~live)
    errs = {'s': float(np.abs(got['seq_logp'][live] - s_want[live]).max()) if live.any() else 0.0,
            'post': float(np.abs(got['post'] - want['post']).max()), 'utt_err': float(np.abs(got['utt_err'] - want['utt_err']).max()),
            'loss': float(np.abs(got['loss3'] - [want['loss'], want['mwer'], want['ctc']]).max()),
            'nll_ref': float(np.abs(got['nll_ref'] - want['nll_ref']).max())}
    print('ctc_mwer %s: |s err| %.3g (eps %.3g), |post err| %.3g, |utt_err err| %.3g, |loss3 err| %.3g (bound %.3g), |nll_ref err| %.3g' % (
        tag, errs['s'], eps, errs['post'], errs['utt_err'], errs['loss'], 4 * eps * w_max, errs['nll_ref']))
    assert np.all(np.abs(got['seq_logp'][live] - s_want[live]) <= 1e-4 + 1e-6 * np.abs(s_want[live]))
    assert np.all(np.abs(got['post'] - want['post']) <= 4 * eps * w_max) and np.all(got['post'][~live] == 0)
    assert np.all(np.abs(got['utt_err'] - want['utt_err']) <= 4 * eps * w_max)
    assert np.all(np.abs(got['loss3'] - [want['loss'], want['mwer'], want['ctc']]) <= 4 * eps * w_max)
    assert np.all(np.abs(got['nll_ref'] - want['nll_ref']) <= 1e-4 + 1e-6 * np.abs(want['nll_ref']))
    d = got['dlogits']
    if d is None:
        return
    err = float(np.abs(d - g * want['grad']).max())
    bound = max(1e-6 * g, 4 * g * want['d0'])
    ratio = err / (g * want['d0']) if want['d0'] > 0 else 0.0
    print('  dlogits: max |err| %.3g, float32 floor d0 %.3g, ratio %.3g, bound %.3g, max |grad| %.3g' % (
        err, g * want['d0'], ratio, bound, g * np.abs(want['grad']).max()))
    _record({'case': tag, 'shape': list(d.shape), 'N': int(live.shape[1]), 'grad_err': err, 'd0': g * want['d0'], 'grad_err_over_d0': ratio,
             'bound': bound, 'max_grad': float(g * np.abs(want['grad']).max()), 's_err': errs['s'], 'post_err': errs['post'],
             'loss_err': errs['loss']})
    assert err <= bound, (tag, err, bound)
    for b in range(d.shape[0]):                                # frames at or past in_len, dead utterances: exactly zero
        Tb = int(np.clip(c['in_len'][b], 0, d.shape[1]))
        assert not d[b, Tb:].any(), (tag, b)
        if not live[b].any() and not want['ok_ref'][b]:
            assert not d[b].any(), (tag, b)


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('N', [1, 2, 5, 32])
@pytest.mark.parametrize('V', [7, 100, 4233])
def test_kernel_matches_restatement(V, N, mode):
    c, dead = _case('main', V, N)
    want = _want('main', V, N, mode)
    with_ref, w, _ = MODES[mode]
    assert c['in_len'][0] == 40 and 0 < c['in_len'][1] < 40 and c['in_len'][3] == 0 and dead[3].all()
    if N >= 5:          # one dead slot of each kind, the repeated label and the empty hypothesis are in
        assert dead[1, N - 3:].all() and dead[2, N - 1] and not dead[0].any() and c['hyp_len'][0, N - 2] == 0
    if N >= 2:          # the test cannot pass on vanishing gradients: a third of the live slots carry |P (W - E)| above 1e-3
        carry = np.abs(want['post'] * (c['errors'] - want['utt_err'][:, None]))[want['live']] > cases.CARRY
        assert carry.sum() * 3 >= want['live'].sum(), (carry.sum(), want['live'].sum())
    tag = 'V%d N%d %s' % (V, N, mode)
    got = _run(c, mode)
    _check(tag, c, got, want)
    again = _run(c, mode)
    fwd = _run(c, mode, grad=False)
    for k in SCALARS:
        assert np.array_equal(got[k], again[k]), k              # the same bits on every run
        assert np.array_equal(got[k], fwd[k]), k                # dlogits = NULL: the same scalar outputs, bit for bit
    if N == 1 and (not with_ref or w == 0):
        assert not got['dlogits'].any()                         # one hypothesis: its errors, and no gradient anywhere
        assert got['loss3'][1] == c['errors'][want['live']].mean()
    if N == 5 and V == 100:
        scaled = _run(c, mode, gscale=torch.tensor([1024.0], device=DEV))
        _check(tag + ' g1024', c, scaled, want, g=1024.0)
        assert np.array_equal(scaled['loss3'], got['loss3'])


@pytest.mark.parametrize('mode', ['noref', 'w0.3'])
def test_all_states_of_the_workgroup(mode):
    """B 2, T 300, V 100, N 5, 127 labels: S = 255; and a slot of 128 labels in rows that hold them is dead by the bound alone"""
    c, dead = _case('big')
    want = _want('big', 0, 0, mode)
    assert c['hyp_len'].max() == 128 and dead.sum() == 1 and (c['hyp_len'][~dead] == 127).all() and c['hyps'].shape[2] == 130
    assert (np.abs(want['c'][want['live']]) > 1e-3 / 2).all()
    _check('big %s' % mode, c, _run(c, mode), want)


@pytest.mark.parametrize('mode', ['noref', 'w0.3'])
def test_unaligned_gradient_and_odd_slabs(mode):
    """the scalar-store path: the gradient's base one float behind an aligned address; and T * V odd, where the utterances' slabs
    of log_probs and of the gradient start off a 16-byte boundary and end inside a quad"""
    c, _ = _case('main', 100, 5)
    want = _want('main', 100, 5, mode)
    base = _run(c, mode)
    off = _run(c, mode, offset=1)
    _check('V100 N5 %s offset 1' % mode, c, off, want)
    for k in SCALARS:
        assert np.array_equal(base[k], off[k]), k
    c, _ = _case('odd', 7, 5)
    assert (c['logits'].shape[1] * c['logits'].shape[2]) % 2 == 1
    _check('T39 V7 N5 %s' % mode, c, _run(c, mode), _want('odd', 7, 5, mode))
    _check('T39 V7 N5 %s offset 1' % mode, c, _run(c, mode, offset=1), _want('odd', 7, 5, mode))


def test_without_a_live_slot_it_is_the_ctc_loss():
    """errors < 0 everywhere, a reference, ctc_weight 1: dlogits and ctc against otr_ctc_loss on the same tensors, within what
    tests/test_gpu_ctc_loss.py allows between two launches of one computation: nll bit-equal, slabs within 2 tiny_b of each other
    (relative, per utterance), the scalar equal up to the order of B float32 additions"""
    from opentransformer_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    c, _ = _case('main', 100, 5)
    B, T, V = c['logits'].shape
    got = _run(c, 'w0.3', errors=np.full_like(c['errors'], -1), ctc_weight=1.0)
    assert not got['post'].any() and np.all(got['seq_logp'] == -np.inf) and got['loss3'][1] == 0 and got['loss3'][0] == got['loss3'][2]
    W = c['ref'].shape[1]
    rf, rl, il = _dev(c['ref']), _dev(c['ref_len'].astype(np.int32)), _dev(c['in_len'].astype(np.int32))
    ws, nll, loss = torch.empty(B, T, 2 * W + 1, device=DEV), torch.empty(B, device=DEV), torch.empty((), device=DEV)
    dl = torch.full((B, T, V), float('nan'), device=DEV)
    rc = lib.otr_ctc_loss(p(got['lp']), p(rf), W, p(il), p(rl), B, T, V, W, cases.BLANK, p(ws), p(nll), p(loss), p(dl),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.otr_last_error_string()
    torch.cuda.synchronize()
    assert np.array_equal(got['nll_ref'], nll.cpu().numpy()) and float(loss) > 0
    assert abs(float(got['loss3'][2]) - float(loss)) <= B * cc.EPS32 * abs(float(loss))
    tn = cc.tiny(torch.from_numpy(c['logits']), torch.from_numpy(c['in_len']))
    a, b = torch.from_numpy(got['dlogits']).double(), dl.cpu().double()
    for u in range(3):                                          # utterance 3 has no frames: both slabs are zero
        assert float((a[u] - b[u]).norm()) <= 2 * float(tn[u]) * float(b[u].norm()), u
    assert float(b[0].norm()) > 0 and not a[3].any() and not b[3].any()


# ---------------------------------------------------------------- the op
def test_op_reads_views_in_place_and_backward_scales():
    """ops.ctc_mwer_loss on the search's kind of rows (wider than any hypothesis, padded with -1) and on a strided reference view
    gives the entry's outputs; only the loss carries a gradient, and backward multiplies the saved one by its seed"""
    from opentransformer_amd import ops
    c, _ = _case('main', 100, 5)
    want = _want('main', 100, 5, 'w0.3')
    B, T, V = c['logits'].shape
    x = _dev(c['logits'].astype(np.float32)).requires_grad_(True)
    wide = torch.full((B, 5, 140), -1, dtype=torch.int64, device=DEV)
    wide[:, :, :8] = _dev(c['hyps'])
    truth = torch.full((B, 10), 1, dtype=torch.int64, device=DEV)
    truth[:, 1:9] = _dev(c['ref'])
    loss, st = ops.ctc_mwer_loss(x, _dev(c['in_len']).long(), wide[:, :, :130], _dev(c['hyp_len']), _dev(c['errors']), ref=truth[:, 1:-1],
                                 ref_len=_dev(c['ref_len']), ctc_weight=0.3)
    assert loss.requires_grad and not any(v.requires_grad for v in st.values())
    (g,) = torch.autograd.grad(3.0 * loss, x)
    torch.cuda.synchronize()
    got = {'loss3': np.array([loss.item(), st['mwer'].item(), st['ctc'].item()], np.float32), 'seq_logp': st['seq_logp'].cpu().numpy(),
           'post': st['post'].cpu().numpy(), 'utt_err': st['utt_err'].cpu().numpy(), 'nll_ref': want['nll_ref'].astype(np.float32),
           'dlogits': g.cpu().numpy()}
    _check('op V100 N5 w0.3 seed 3', c, got, want, g=3.0)
    direct = _run(c, 'w0.3')
    for k in ('loss3', 'seq_logp', 'post', 'utt_err'):
        assert np.array_equal(got[k], direct[k]), k
    fwd, _ = ops.ctc_mwer_loss(x.detach(), _dev(c['in_len']), _dev(c['hyps']), _dev(c['hyp_len']), _dev(c['errors']))
    assert not fwd.requires_grad and fwd.item() == _run(c, 'noref', grad=False)['loss3'][0]


# ---------------------------------------------------------------- the trainer
def _model_case():
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ops.set_compute_dtype('fp32')
    cfg = syn.c1_model(0.0)                                     # the smallest CTCModel tests/test_model_passes.py builds
    V = cfg['decoder']['vocab_size']
    model = ota.CTCModel(dict(cfg, vocab_size=V))
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).train()
    inputs, targets = syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=V, tgt_len=4, seed=0)
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    labels = targets['targets'][:, 1:-1]
    L = 20                                                      # more labels than the 15 encoder frames of 64 input frames
    tokens = torch.full((2, 3, L), -1, dtype=torch.int64, device=DEV)
    tokens[:, 0, :4] = labels                                   # the reference itself
    bad = labels.clone()
    for j in (1, 3):                                            # a copy with two substitutions
        bad[:, j] = 3 + (bad[:, j] + 5) % (V - 3)
    tokens[:, 1, :4] = bad
    tokens[:, 2] = torch.randint(3, V, (2, L), generator=torch.Generator().manual_seed(7)).to(DEV)
    lengths = torch.tensor([[4, 4, L]] * 2, dtype=torch.int32, device=DEV)
    return model, inputs, targets, (tokens, lengths), V


def _composed_step(model, inputs, targets, hyps, ctc_weight, dtype):
    """CTCMWERTraining.forward with the loss (and only the loss) composed from torch ops in `dtype`, on the CPU, on the model's own
    logits; its gradient into the logits goes back through the model's own backward.  Returns (loss, mwer, logits, d loss / d logits)."""
    from opentransformer_amd import ops
    tokens, lengths = hyps
    labels, labels_length = targets['targets'][:, 1:-1], targets['targets_length'] - 1
    errors = ops.edit_distance(labels, labels_length, tokens, lengths)[0]
    memory, memory_mask = model.encode(inputs['inputs'], inputs['mask'])
    logits = model.assistor(memory, return_logits=True)
    c = {'logits': logits.detach().double().cpu().numpy(), 'in_len': memory_mask.sum(-1).cpu().numpy(), 'hyps': tokens.cpu().numpy(),
         'hyp_len': lengths.cpu().numpy(), 'errors': errors.cpu().numpy(), 'ref': labels.cpu().numpy(), 'ref_len': labels_length.cpu().numpy()}
    live = ref.forward(c['logits'], c['in_len'], c['hyps'], c['hyp_len'], c['errors'])['live']
    loss, mwer, _, d = cases.compose_torch(c, live, ctc_weight, 1.0, True, dtype)
    return loss, mwer, logits, torch.from_numpy(d).to(DEV).float(), errors, live


def _grads(model, run):
    for p in model.parameters():
        p.grad = None
    run()
    torch.cuda.synchronize()
    named = [(n, p.grad.detach().clone()) for n, p in model.named_parameters() if p.grad is not None]
    return [n for n, _ in named], [g for _, g in named]


@pytest.mark.parametrize('ctc_weight', [0.01, 0.0])
def test_training_step_matches_the_composed_loss(ctc_weight):
    """fp32 mode.  The loss to six digits; the parameter gradients (tests.helpers.key_aware_grad_errors) under max(1e-4, 4 d0), d0 the
    distance between the composed route with float32 and with float64 loss math, as tests/test_gpu_mwer.py holds MWERTraining"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, hyps, V = _model_case()
        modes = [m.training for m in model.modules()]
        wrap = ota.CTCMWERTraining(model, nbest=3, ctc_weight=ctc_weight)
        loss, aux = wrap(inputs, targets, hyps=hyps)
        names, got = _grads(model, lambda: ops.backward(loss))
        loss64, mwer64, logits, d64, errors, live = _composed_step(model, inputs, targets, hyps, ctc_weight, torch.float64)
        names64, want = _grads(model, lambda: torch.autograd.backward(logits, grad_tensors=d64))
        _, _, logits, d32, _, _ = _composed_step(model, inputs, targets, hyps, ctc_weight, torch.float32)
        _, base = _grads(model, lambda: torch.autograd.backward(logits, grad_tensors=d32))
        assert names == names64 and len(names) > 10 and [m.training for m in model.modules()] == modes
        assert live.tolist() == [[True, True, False]] * 2       # the slot with more labels than frames takes no part
        assert torch.equal(aux['errors_1best'], errors[:, 0]) and int(errors[:, 0].abs().sum()) == 0 and bool((errors[:, 1] == 2).all())
        assert torch.equal(aux['errors_oracle'], errors[:, :2].min(dim=1).values)
        assert bool((aux['post'][:, 2] == 0).all()) and bool((aux['post'][:, :2] > 0).all())
        print('ctc_mwer model ctc_weight=%g: posteriors %s; MWER %.7f composed %.7f, total %.7f composed %.7f' % (
            ctc_weight, aux['post'][:, :2].tolist(), float(aux['MWER']), mwer64.item(), loss.item(), loss64.item()))
        assert int((aux['post'][:, :2].min(dim=1).values > 1e-2).sum()) >= 1      # a split posterior: the weights do not vanish
        assert abs(loss.item() - loss64.item()) <= 1e-6 * abs(loss64.item()) and abs(float(aux['MWER']) - mwer64.item()) <= 1e-6 * mwer64.item()
        d_model = syn.c1_model(0.0)['encoder']['d_model']
        errs, _ = H.key_aware_grad_errors(names, got, want, d_model)
        d0, _ = H.key_aware_grad_errors(names, base, want, d_model)
        worst = max(errs, key=lambda k: errs[k] / max(1e-4, 4 * d0[k]))
        print('  grads: worst %s err %.3g bound %.3g; max err %.3g, max d0 %.3g' % (
            worst, errs[worst], max(1e-4, 4 * d0[worst]), max(errs.values()), max(d0.values())))
        assert len(errs) > 10
        for k, e in errs.items():
            assert e <= max(1e-4, 4 * d0[k]), (k, e, d0[k])
    finally:
        ops.set_compute_dtype('bf16')


def test_search_inside_the_step(monkeypatch):
    """hyps=None: the n-best is the beam search's own (errors_1best is the edit distance of CTCRecognizer(mode='beam')'s 1-best), one
    encoder pass with a gradient, the modes restored, everything finite, and a second step after a weight update runs"""
    import opentransformer_amd as ota
    from opentransformer_amd import model as M
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import CTCRecognizer
    try:
        model, inputs, targets, _, V = _model_case()
        modes = [m.training for m in model.modules()]
        wrap = ota.CTCMWERTraining(model, nbest=3, beam_width=4, ctc_weight=0.01)
        assert [m.training for m in model.modules()] == modes
        with torch.no_grad(), M.evaluating(model):
            tokens, lengths, _ = CTCRecognizer(model, mode='beam', beam_width=4).recognize_tokens(inputs['inputs'], inputs['mask'])
        assert [m.training for m in model.modules()] == modes
        best = ops.edit_distance(targets['targets'][:, 1:-1], targets['targets_length'] - 1, tokens, lengths)[0][:, 0]
        calls = []
        encode = M.AcousticModel.encode

        def counting(self, inputs, inputs_mask, mark=False):
            calls.append((type(self).__name__, mark, torch.is_grad_enabled()))
            return encode(self, inputs, inputs_mask, mark)
        monkeypatch.setattr(M.AcousticModel, 'encode', counting)
        for step in range(2):
            calls.clear()
            loss, aux = wrap(inputs, targets)
            assert calls == [('CTCModel', False, True)]            # the one encoder pass of the step
            for p in model.parameters():
                p.grad = None
            ops.backward(loss)
            torch.cuda.synchronize()
            assert [m.training for m in model.modules()] == modes
            assert aux['post'].shape == (2, 3) and set(aux) == {'MWER', 'CTC', 'errors_1best', 'errors_oracle', 'post'}
            assert all(bool(torch.isfinite(v.float()).all()) for v in aux.values()) and bool(torch.isfinite(loss))
            grads = [p.grad for p in model.parameters() if p.grad is not None]
            assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
            if step == 0:
                assert torch.equal(aux['errors_1best'], best)
                assert bool((aux['errors_oracle'] <= aux['errors_1best']).all())
                with torch.no_grad():
                    for p in model.parameters():
                        if p.grad is not None:
                            p.add_(p.grad, alpha=-0.01)
    finally:
        ops.set_compute_dtype('bf16')
