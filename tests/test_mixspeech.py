"""CPU (-m "not gpu"): MixSpeech.  The host restatement (tests/mixspeech_ref.py) is the torch expression of the reference's trainer; the
named CTC pairs are what tests/test_gpu_mixspeech.py takes them for; the library's entries, ops.mixspeech_mix / ops.ctc_loss_pair and
MixSpeechTraining refuse what is outside the documented limits before they look at the device; and the oracle composite
lam * oracle(mixed, t1) + (1 - lam) * oracle(mixed, t2) is one MixSpeech step of the REAL reference (tests/golden/mixspeech_c1.npz,
written by tests/make_mixspeech_golden.py)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from opentransformer_amd import synthetic as syn
from tests import ctc_loss_cases as cc
from tests import helpers as H
from tests import mixspeech_ref as ref

BATCH = dict(batch=5, frames=96, feat_dim=80, vocab=100, tgt_len=6, seed=7, lengths=[96, 80, 96, 64, 50], tgt_lengths=[6, 4, 5, 6, 3])


def test_binding_and_header_carry_the_entries():
    header = (Path(__file__).resolve().parent.parent / 'include' / 'otrans_hip.h').read_text()
    assert 'otr_mixspeech_mix and otr_ctc_loss_pair (additions only)' in header
    assert 'int32_t otr_mixspeech_mix(' in header and 'int32_t otr_ctc_loss_pair(' in header
    assert len(_lib.SIGNATURES['otr_mixspeech_mix']) == 11 and len(_lib.SIGNATURES['otr_ctc_loss_pair']) == 19
    for kind in ('bf16', 'fp16'):
        assert hasattr(_lib.load(kind), 'otr_mixspeech_mix') and hasattr(_lib.load(kind), 'otr_ctc_loss_pair')


def test_entry_points_refuse_bad_arguments_and_leave_the_outputs_alone():
    """checked on the host before any launch (no GPU needed): every output buffer still holds its fill afterwards"""
    lib = _lib.load()
    fill = 123.25
    bufs = {k: (C.c_float * 64)(*([fill] * 64)) for k in ('out', 'len', 'mask', 'ws', 'nll', 'loss', 'dl')}
    p = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}
    inp = C.cast((C.c_float * 64)(), C.c_void_p)

    def mix(x=inp, pitch=6, lengths=inp, lam=inp, B=2, T=3, F=2, out=p['out'], out_len=p['len'], mask=p['mask']):
        return lib.otr_mixspeech_mix(x, pitch, lengths, lam, B, T, F, out, out_len, mask, None)
    for kw in [dict(B=1), dict(B=0), dict(B=-2), dict(T=0), dict(F=0), dict(T=-1), dict(F=-3), dict(x=None), dict(lengths=None),
               dict(lam=None), dict(out=None), dict(out_len=None), dict(mask=None), dict(pitch=5), dict(T=1 << 16, F=1 << 15, pitch=1 << 40),
               dict(B=1 << 18)]:
        assert mix(**kw) < 0, kw
        assert b'mixspeech_mix' in lib.otr_last_error_string(), kw

    def pair(lp=inp, ta=inp, lda=4, la=inp, tb=inp, ldb=4, lb=inp, il=inp, lam=inp, P=2, T=3, V=5, max_tgt=4, blank=0, ws=p['ws'],
             nll=p['nll'], loss=p['loss'], dl=p['dl']):
        return lib.otr_ctc_loss_pair(lp, ta, lda, la, tb, ldb, lb, il, lam, P, T, V, max_tgt, blank, ws, nll, loss, dl, None)
    for kw in [dict(lp=None), dict(ta=None), dict(tb=None), dict(la=None), dict(lb=None), dict(il=None), dict(lam=None), dict(ws=None),
               dict(nll=None), dict(loss=None), dict(P=0), dict(P=-1), dict(P=1 << 16), dict(T=0), dict(V=1), dict(max_tgt=128, lda=128, ldb=128),
               dict(max_tgt=-1), dict(lda=3), dict(ldb=3), dict(blank=5), dict(blank=-1)]:
        assert pair(**kw) < 0, kw
        assert b'ctc_loss_pair' in lib.otr_last_error_string(), kw
    assert b'127' in (pair(max_tgt=128, lda=128, ldb=128), lib.otr_last_error_string())[1]
    for k, b in bufs.items():
        assert all(v == fill for v in b), k


def test_ops_refuse_before_they_look_at_the_device():
    from opentransformer_amd import ops
    x, n, lam = torch.zeros(4, 5, 3), torch.tensor([5, 4, 3, 2]), torch.tensor([0.3])
    for bad in (dict(x=x[:1]), dict(x=x[0]), dict(x=torch.zeros(4, 0, 3)), dict(x=torch.zeros(4, 5, 0)), dict(n=n[:3]), dict(lam=0.3),
                dict(lam=torch.tensor([0.3, 0.4]))):
        kw = dict(dict(x=x, n=n, lam=lam), **bad)
        with pytest.raises(ValueError, match='mixspeech_mix'):
            ops.mixspeech_mix(kw['x'], kw['n'], kw['lam'])
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):      # well-formed arguments: the next check is the device
        ops.mixspeech_mix(x, n, lam)
    P, T, V, W = 2, 6, 7, 3
    lg, tg, il, tl = torch.zeros(P, T, V), torch.ones(P, W, dtype=torch.int64), torch.tensor([6, 6]), torch.tensor([3, 2])
    good = dict(lg=lg, ta=tg, tb=tg, il=il, la=tl, lb=tl, lam=lam, blank=0)
    for bad in (dict(lg=lg[0]), dict(lg=torch.zeros(P, T, 1)), dict(lg=torch.zeros(P, 0, V)), dict(ta=tg[:1]), dict(tb=tg[:, :2]), dict(ta=tg[0]),
                dict(ta=torch.ones(P, 128, dtype=torch.int64), tb=torch.ones(P, 128, dtype=torch.int64)), dict(il=il[:1]), dict(la=tl[:1]),
                dict(lb=torch.tensor([1, 2, 3])), dict(lam=0.3), dict(lam=torch.tensor([0.3, 0.4])), dict(blank=V), dict(blank=-1)):
        kw = dict(good, **bad)
        with pytest.raises(ValueError, match='ctc_loss_pair'):
            ops.ctc_loss_pair(kw['lg'], kw['ta'], kw['tb'], kw['il'], kw['la'], kw['lb'], kw['lam'], kw['blank'])
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):
        ops.ctc_loss_pair(lg, tg, tg, il, tl, tl, lam)


def test_wrapper_refuses_bad_settings_and_shows_the_models_parameters():
    import opentransformer_amd as ota
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    for alpha in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='MixSpeechTraining'):
            ota.MixSpeechTraining(model, alpha=alpha)
    with pytest.raises(ValueError, match='MixSpeechTraining'):
        ota.MixSpeechTraining(torch.nn.Linear(3, 3))
    wrap = ota.MixSpeechTraining(model)
    assert wrap.alpha == 0.5 and wrap.model is model
    assert [k for k, _ in wrap.named_parameters()] == ['model.' + k for k, _ in model.named_parameters()]
    assert sorted(wrap.state_dict()) == sorted('model.' + k for k in model.state_dict())
    inputs, targets = syn.synthetic_batch(1, 40, 80, 100, 4)
    with pytest.raises(ValueError, match='MixSpeechTraining'):             # B < 2: no pair, refused before the device is touched
        wrap.train()(inputs, targets)
    # the draw is the reference's call on numpy's global generator
    np.random.seed(31)
    want = np.float32(np.random.beta(0.5, 0.5, size=(1))[0])
    np.random.seed(31)
    assert wrap.draw() == want and wrap.draw().dtype == np.float32


# ------------------------------------------------------------------------------------------ the mix
def _torch_mix(x, mask, lengths, lam):
    """what trainer.py:163-182 computes, on zero-padded input: a [P, T, F] tensor of lam, even * c + odd * (1 - c), torch.max of the masks
    and lengths"""
    x, mask, lengths = torch.from_numpy(x), torch.from_numpy(mask), torch.from_numpy(lengths)
    n = x.shape[0] // 2 * 2
    c = torch.from_numpy(np.asarray([lam], np.float64)).float().unsqueeze(1).unsqueeze(1).repeat(n // 2, x.shape[1], x.shape[2])
    return (x[0:n:2] * c + x[1:n:2] * (1 - c), torch.max(mask[0:n:2], mask[1:n:2]), torch.max(lengths[0:n:2], lengths[1:n:2]))


@pytest.mark.parametrize('lam', [0.0, 1.0, 0.5, 0.3, 'beta'])
@pytest.mark.parametrize('B,T,F', [(2, 1, 1), (3, 7, 3), (5, 96, 80), (8, 7, 83)])
def test_mix_pairs_is_the_torch_expression_of_the_trainer(B, T, F, lam):
    rng = np.random.default_rng(B * 1000 + T * 10 + F)
    if lam == 'beta':
        np.random.seed(B + T + F)
        lam = np.random.beta(0.5, 0.5, size=(1))[0]
    lengths = rng.integers(0, T + 1, B)
    lengths[0] = T
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    mask = np.arange(T)[None, :] < lengths[:, None]
    x[~mask] = 0.0                                                       # the collate's zero padding
    want, want_mask, want_len = _torch_mix(x, mask, lengths, lam)
    got, got_len, got_mask = ref.mix_pairs(x, lengths, np.float32(lam))
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert np.array_equal(got_mask, want_mask.numpy()) and np.array_equal(got_len, want_len.numpy())
    poisoned = np.where(mask[:, :, None], x, np.float32('nan'))           # padding that is not zero cannot leak in
    again, _, _ = ref.mix_pairs(poisoned, lengths, np.float32(lam))
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------ the CTC pairs
def _feas(name):
    a, b = ref.pair_of(name)
    return list(zip([int(f) for f in cc.feasible(a)], [int(f) for f in cc.feasible(b)]))


def test_named_ctc_pairs_are_what_they_claim():
    assert _feas('one_frame_short') == [(0, 1), (1, 1), (0, 1), (1, 0)]
    es = _feas('empty_and_short')
    assert es[2] == (0, 0) and es[3] == (0, 0) and es[6] == (0, 1)
    assert _feas('tgt_len_guard') == [(1, 1), (0, 1), (1, 0), (0, 1), (0, 0), (0, 0), (1, 0)]
    for name in ('waves_v50', 'straddle_on', 'ragged_in_len', 'blank_mid', 'peaked_x4'):
        assert all(f == (1, 1) for f in _feas(name)), name
    a, b = ref.pair_of('waves_v50')
    assert b['logits'] is a['logits'] and b['in_len'] is a['in_len']
    assert torch.equal(b['targets'][1:], a['targets'][:-1]) and torch.equal(b['targets'][0], a['targets'][-1])
    assert torch.equal(b['tgt_len'][1:], a['tgt_len'][:-1])


def test_ctc_pair_is_the_weighted_sum_of_the_two_references():
    name, lam = 'one_frame_short', 0.3
    a, b = ref.pair_of(name)
    r = ref.reference_of(name, lam)
    la, na, ga = cc.reference_of(name)
    assert torch.equal(r['loss_a'], la) and torch.equal(r['nll'][0], na) and torch.equal(r['g_a'], ga)
    l32, o32 = float(np.float32(lam)), float(np.float32(1) - np.float32(lam))
    assert abs(float(r['loss']) - (l32 * float(r['loss_a']) + o32 * float(r['loss_b']))) < 1e-12
    fa, fb = cc.feasible(a), cc.feasible(b)
    for p in range(4):                                                   # an infeasible set contributes nothing to the slab
        want = l32 * r['g_a'][p] * fa[p] + o32 * r['g_b'][p] * fb[p]
        assert float((r['grad'][p] - want).abs().max()) < 1e-15
        assert float(r['nll'][0, p]) == 0.0 or fa[p]
        assert float(r['nll'][1, p]) == 0.0 or fb[p]
    fl = ref.floor_of(name, lam)
    assert tuple(fl['nll'].shape) == (2, 4) and tuple(fl['grad'].shape) == (4,) and fl['loss'] < 1e-5


# ------------------------------------------------------------------------------------------ the reference's own step
@pytest.mark.parametrize('kind', ['att', 'joint'])
def test_oracle_composite_matches_the_reference_step(golden, kind):
    """the bars tests/test_oracle_golden.py uses for the other c1 fixtures (rtol 2e-5 on the loss, 5 rtol on gradient norm and probe)"""
    g = golden('mixspeech_c1.npz')
    rtol = 2e-5
    cfg = syn.c1_model(0.0, ctc_weight=0.3 if kind == 'joint' else 0.0)
    inputs, targets = syn.synthetic_batch(**BATCH)
    lam = np.float32(g[kind + '_lambda'][0])
    np.random.seed(int(g['seed']))
    assert np.float32(np.random.beta(0.5, 0.5, size=(1))[0]) == lam      # the stored lambda is the seeded draw
    loss, loss_1, loss_2, parts = ref.oracle_composite(cfg, inputs, targets, lam)
    for got, key in ((loss, 'loss'), (loss_1, 'loss_1'), (loss_2, 'loss_2')):
        want = float(g['%s_%s' % (kind, key)])
        assert abs(got.item() - want) <= rtol * abs(want), (key, got.item(), want)
    flat = H.flat_named(parts)
    loss.backward()
    seen = set()
    keys = [str(k) for k in g[kind + '_grad_keys']]
    assert len(keys) > 10
    for k, (nrm, dot) in zip(keys, g[kind + '_grad_summary']):
        t = flat[k]
        if t.data_ptr() in seen:
            continue
        seen.add(t.data_ptr())
        gr = t.grad.double().reshape(-1).numpy()
        assert abs(np.sqrt((gr * gr).sum()) - nrm) <= 5 * rtol * max(nrm, 1e-6), k
        assert abs((gr * H.probe_vector(k, gr.size)).sum() - dot) <= 5 * rtol * max(nrm * np.sqrt(gr.size), 1e-6), k
    # the fifth utterance was dropped: other features and targets there change nothing
    inputs2 = {k: v.clone() for k, v in inputs.items()}
    inputs2['inputs'][4] += 1.0
    again = ref.oracle_composite(cfg, inputs2, targets, lam)[0]
    assert again.item() == loss.item()
