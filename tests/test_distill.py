"""CPU (-m "not gpu"): knowledge distillation.  The numpy restatement (tests/distill_ref.py) is the loss torch composes from kl_div,
dense and top-K; the library's entry points, ops.distill_loss / distill_loss_topk / topk_rows and DistillTraining refuse what is
outside the documented limits before they look at the device; the teacher stays out of the wrapper's parameters."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opentransformer_amd import _lib
from tests import distill_ref as ref


def _torch_loss(s, t_logits, live, tau):
    """tau^2 * kl_div(log_softmax(s / tau), softmax(t / tau), 'sum') / n_live over the live rows, and its autograd gradient"""
    s = torch.from_numpy(np.asarray(s, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(t_logits, np.float64))
    m = torch.from_numpy(live)
    loss = tau * tau * F.kl_div(torch.log_softmax(s[m] / tau, -1), torch.softmax(t[m] / tau, -1), reduction='sum') / int(live.sum())
    loss.backward()
    return loss.item(), s.grad.numpy()


@pytest.mark.parametrize('tau', [0.5, 1.0, 2.0, 4.0])
@pytest.mark.parametrize('V', [37, 4233])
def test_restatement_is_the_kl_div_of_torch(V, tau):
    rng = np.random.default_rng(V + int(8 * tau))
    B, T, K = 3, 7, 8
    s, t = ref.case(rng, B, T, V)
    lengths = np.array([9, -2, 3])
    want = ref.forward(s, lengths, V, tau, teacher=t)
    assert want['n_live'] == 10 and want['live'][0].all() and not want['live'][1].any() and want['live'][2].sum() == 3
    assert want['row_kl'][want['live']].mean() >= 0.01                      # a signal that does not vanish
    loss, grad = _torch_loss(s, t, want['live'], tau)
    assert abs(want['loss'] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(want['grad'] - grad).max() <= 1e-12
    assert not want['grad'][~want['live']].any() and not want['row_kl'][~want['live']].any()
    # top-K: the teacher's distribution is the softmax over the listed entries, zero elsewhere -- a dense teacher of -inf off the list
    val, idx = ref.topk(t, K)
    sparse = ref.forward(s, lengths, V, tau, top_val=val, top_idx=idx)
    masked = np.full(t.shape, -np.inf)
    np.put_along_axis(masked, idx.astype(np.int64), val.astype(np.float64), axis=-1)
    loss_k, grad_k = _torch_loss(s, masked, sparse['live'], tau)
    assert abs(sparse['loss'] - loss_k) <= 1e-12 * max(1.0, abs(loss_k)) and np.abs(sparse['grad'] - grad_k).max() <= 1e-12
    dense_inf = ref.forward(s, lengths, V, tau, teacher=masked)
    assert abs(dense_inf['loss'] - sparse['loss']) <= 1e-12 and np.isfinite(dense_inf['grad']).all()


def test_restatement_edges():
    rng = np.random.default_rng(5)
    B, T, V = 3, 7, 5
    s, t = ref.case(rng, B, T, V)
    none = ref.forward(s, np.zeros(3, np.int64), V, 2.0, teacher=t)
    assert none['n_live'] == 0 and none['loss'] == 0 and not none['grad'].any()
    same = ref.forward(s, [7, 7, 7], V, 2.0, teacher=s)
    assert np.abs(same['row_kl']).max() < 1e-14 and np.abs(same['grad']).max() < 1e-16
    # indices outside [0, V) drop their entries; a row that lists nothing is dead
    val = rng.normal(size=(B, T, 8)).astype(np.float32)
    idx = np.tile(np.array([0, -1, 1, V, 2, 1 << 30, 3, -(1 << 31)], np.int64), (B, T, 1)).astype(np.int32)
    idx[0, 2] = [-1, V, V + 1, -7, 99, 1 << 20, -(1 << 31), V]
    f = ref.forward(s, [7, 7, 7], V, 1.0, top_val=val, top_idx=idx)
    assert not f['live'][0, 2] and f['n_live'] == 20 and not f['q'][:, :, 4].any() and abs(f['q'][1, 1].sum() - 1) < 1e-12
    g3 = ref.forward(s, [7, 0, 3], V, 2.0, teacher=t, g=3.0)
    g1 = ref.forward(s, [7, 0, 3], V, 2.0, teacher=t)
    assert np.allclose(g3['grad'], 3 * g1['grad'], rtol=1e-15, atol=0)


def test_binding_and_header_carry_the_entries():
    header = (Path(__file__).resolve().parent.parent / 'include' / 'otrans_hip.h').read_text()
    assert 'otr_distill_workspace_floats and otr_distill_loss (additions only)' in header
    assert 'otr_distill_loss' in _lib.SIGNATURES and 'otr_distill_workspace_floats' in _lib.SIGNATURES
    for kind in ('bf16', 'fp16'):
        assert hasattr(_lib.load(kind), 'otr_distill_loss')


def test_workspace_size_and_bad_shapes():
    lib = _lib.load()
    assert lib.otr_distill_workspace_floats(32, 250) == 4 * 32 * 250 + 4
    assert lib.otr_distill_workspace_floats(0, 7) == 4
    for B, T in ((-1, 7), (3, 0), (3, -1), (1 << 15, 1 << 15), (1 << 20, 1 << 10)):
        assert lib.otr_distill_workspace_floats(B, T) == -1, (B, T)


def test_entry_point_refuses_bad_arguments_and_leaves_the_outputs_alone():
    """checked on the host before any launch (no GPU needed): every output buffer still holds its fill afterwards"""
    lib = _lib.load()
    fill = 123.25
    bufs = {k: (C.c_float * 64)(*([fill] * 64)) for k in ('loss', 'kl', 'dl', 'ws')}
    p = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}
    inp = C.cast((C.c_float * 64)(), C.c_void_p)
    need = 4 * 2 * 7 + 4

    def call(s=inp, ld_s=100, t=inp, ld_t=100, tv=None, ti=None, K=0, lengths=inp, B=2, T=7, V=100, tau=2.0, loss=p['loss'], kl=p['kl'],
             dl=p['dl'], ldd=100, ws=p['ws'], nws=1 << 20):
        return lib.otr_distill_loss(s, ld_s, t, ld_t, tv, ti, K, lengths, B, T, V, tau, None, loss, kl, dl, ldd, ws, nws, None)
    sparse = dict(t=None, ld_t=0, tv=inp, ti=inp, K=8)
    bad = [dict(tv=inp, ti=inp, K=8), dict(tv=inp), dict(K=8), dict(t=None),                    # both forms, or neither
           dict(s=None), dict(lengths=None), dict(loss=None), dict(kl=None), dict(sparse, tv=None), dict(sparse, ti=None),
           dict(V=0), dict(V=8193, ld_s=8200, ld_t=8200, ldd=8200), dict(sparse, K=129), dict(sparse, K=-1), dict(t=None, tv=inp, ti=inp, K=0),
           dict(ld_s=99), dict(ld_t=99), dict(ldd=99), dict(T=0), dict(B=-1), dict(B=1 << 15, T=1 << 15),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=float('inf')), dict(tau=float('nan')),
           dict(ws=None), dict(nws=need - 1)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert b'distill' in lib.otr_last_error_string(), kw
    for k, b in bufs.items():
        assert all(v == fill for v in b), k
    assert call(B=0) == 0 and call(B=0, **sparse) == 0            # nothing to do: no launch
    assert call(B=0, tau=3.3e38) == 0 and call(B=0, tau=1e-30) == 0   # every finite temperature above 0 is taken
    assert all(v == fill for v in bufs['loss'])


def test_ops_refuse_before_they_look_at_the_device():
    from opentransformer_amd import ops
    assert ops.DISTILL_MAX_V == 8192 and ops.DISTILL_MAX_K == 128
    B, T, V, K = 2, 5, 10, 4
    s, t, n = torch.zeros(B, T, V), torch.zeros(B, T, V), torch.full((B,), T, dtype=torch.int32)
    tv, ti = torch.zeros(B, T, K), torch.zeros((B, T, K), dtype=torch.int32)
    with pytest.raises(_lib.OtransHipError):                      # CPU tensors: there is no fallback
        ops.distill_loss(s, t, n)
    with pytest.raises(_lib.OtransHipError):
        ops.distill_loss_topk(s, tv, ti, n)
    with pytest.raises(_lib.OtransHipError):
        ops.topk_rows(t, n, K)
    with pytest.raises(ValueError, match='V=9000'):
        ops.distill_loss(torch.zeros(1, 2, 9000), torch.zeros(1, 2, 9000), n[:1])
    with pytest.raises(ValueError, match='V=9000'):
        ops.distill_loss_topk(torch.zeros(1, 2, 9000), tv[:1, :2], ti[:1, :2], n[:1])
    with pytest.raises(ValueError, match='K=129'):
        ops.distill_loss_topk(s, torch.zeros(B, T, 129), torch.zeros((B, T, 129), dtype=torch.int32), n)
    with pytest.raises(ValueError, match='K=11'):
        ops.topk_rows(t, n, 11)                                   # K > V
    with pytest.raises(ValueError, match='teacher'):
        ops.distill_loss(s, t[:, :-1], n)
    with pytest.raises(ValueError, match='top_idx'):
        ops.distill_loss_topk(s, tv, ti[:, :, :-1], n)
    with pytest.raises(ValueError, match='lengths'):
        ops.distill_loss(s, t, n[:1])
    for tau in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            ops.distill_loss(s, t, n, temperature=tau)
    with pytest.raises(ValueError, match=r'\[B, T, V\]'):
        ops.distill_loss(s[0], t[0], n)


def test_wrapper_refuses_bad_settings_and_keeps_the_teacher_out():
    import opentransformer_amd as ota
    from opentransformer_amd import synthetic as syn
    student, teacher = ota.SpeechToText(syn.c1_model(0.0)), ota.SpeechToText(syn.c1_model(0.0))
    for kw, word in ((dict(kd_weight=1.5), 'kd_weight'), (dict(kd_weight=-0.1), 'kd_weight'), (dict(temperature=0.0), 'temperature'),
                     (dict(temperature=-2.0), 'temperature'), (dict(topk=0), 'topk'), (dict(topk=129), 'topk')):
        with pytest.raises(ValueError, match=word):
            ota.DistillTraining(student, teacher, **kw)
    cfg = syn.c1_model(0.0)
    ctc = ota.CTCModel(dict(cfg, vocab_size=cfg['decoder']['vocab_size']))
    with pytest.raises(ValueError, match='CTCModel'):
        ota.DistillTraining(student, ctc)
    other = syn.c1_model(0.0)
    other['decoder'] = dict(other['decoder'], vocab_size=cfg['decoder']['vocab_size'] + 3)
    with pytest.raises(ValueError, match='V='):
        ota.DistillTraining(student, ota.SpeechToText(other))
    with pytest.raises(ValueError, match='student'):
        ota.DistillTraining(torch.nn.Linear(2, 2), teacher)
    teacher.train()
    wrap = ota.DistillTraining(student, teacher, kd_weight=0.3, temperature=2.0, topk=40)
    assert wrap.model is student and wrap.teacher is teacher and not teacher.training and wrap.topk == 40
    assert [n for n, _ in wrap.named_parameters()] == ['model.' + n for n, _ in student.named_parameters()]
    assert sorted(wrap.state_dict()) == sorted('model.' + k for k in student.state_dict())
    mine = {id(p) for p in wrap.parameters()}
    assert not any(id(p) in mine for p in teacher.parameters())
    assert all(m is not teacher for m in wrap.modules())
    wrap.train()
    assert student.training and not teacher.training
    with pytest.raises(ValueError, match='teacher'):              # neither a teacher nor teacher_out
        ota.DistillTraining(student)({'inputs': None, 'mask': None}, {'targets': None, 'targets_length': None})
    assert wrap.set_epoch(3) is None
