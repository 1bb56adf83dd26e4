"""GPU (-m gpu): knowledge distillation.  otr_distill_loss (csrc/distill.hip) against the numpy float64 restatement
(tests/distill_ref.py) on the 16-byte and the scalar routes, dense and top-K; ops.distill_loss through autograd; DistillTraining against
the same model with the distillation term composed from torch ops in float64 on the model's own logits.

Bounds (the idiom of tests/test_gpu_mwer.py): d0 is the distance, on the same case, between the restatement run in float32 and in
float64 -- what fp32 rounding alone does; the kernel gets 4 x that for its other summation order and the device exp.
  row_kl:   |err| <= 4 max(d0_kl, 1e-6)                       loss: tau^2 times that
  gradient: u = dlogits n_live / (g tau) against p - q, |err| <= 4 max(d0_g, 2e-6) (p + q) elementwise, d0_g = max |err_f32| / (p + q):
            relative to p + q, so an error in either distribution cannot hide under an absolute floor."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import distill_ref as ref
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, T = 3, 7
LENGTHS = {'plain': (7, 0, 3), 'clamped': (9, -2, 1)}
# (V, student pad): teacher pad, gradient pad.  Padded tensors are passed as views: 4240 = 4233 + 7 and 104 = 100 + 4 keep 16-byte rows,
# 8195 does not; at V = 4234 the student (4240) and the teacher (4236) take the 16-byte route and the gradient (4234) the scalar one
PADS = {(5, 0): (0, 0), (37, 0): (0, 0), (100, 4): (4, 4), (4233, 7): (7, 7), (4234, 6): (2, 0), (8192, 0): (0, 0), (8192, 3): (3, 3)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _view(a, V):
    d = _dev(a)
    return d[..., :V] if a.shape[-1] != V else d


@functools.lru_cache(maxsize=None)
def _case(V, pad, tau, which):
    """tests/distill_ref.case and what the restatement makes of it in float64 and float32, once per case"""
    pad_t, _ = PADS[(V, pad)]
    rng = np.random.default_rng(V * 100 + pad * 7 + int(8 * tau))
    s, t = ref.case(rng, B, T, V, pad, pad_t)
    lengths = np.array(LENGTHS[which], np.int32)
    return s, t, lengths, ref.forward(s, lengths, V, tau, teacher=t), ref.forward(s, lengths, V, tau, teacher=t, dtype=np.float32)


def _run(s_d, V, lengths, tau, teacher=None, top=None, grad=True, gscale=None, ldd=None, dl_shift=0):
    """otr_distill_loss through the library's own entry: the tensors as they are (views keep their row stride), every output pre-filled
    with NaN; returns the outputs as numpy arrays (dlogits at its full width).  dl_shift: the gradient buffer starts that many floats
    behind a 16-byte boundary"""
    from opentransformer_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    Bn, Tn = s_d.shape[:2]
    ldd = V if ldd is None else ldd
    loss = torch.full((1,), float('nan'), device=DEV)
    row_kl = torch.full((Bn, Tn), float('nan'), device=DEV)
    dl = torch.full((Bn * Tn * ldd + dl_shift,), float('nan'), device=DEV)[dl_shift:].view(Bn * Tn, ldd) if grad else None
    nws = lib.otr_distill_workspace_floats(Bn, Tn)
    assert nws == 4 * Bn * Tn + 4
    ws = torch.full((nws,), float('nan'), device=DEV)
    tv, ti = top if top is not None else (None, None)
    assert s_d.stride(2) == 1 and s_d.stride(0) == Tn * s_d.stride(1) and (teacher is None or teacher.stride(0) == Tn * teacher.stride(1))
    rc = lib.otr_distill_loss(p(s_d), s_d.stride(1), p(teacher), teacher.stride(1) if teacher is not None else 0, p(tv), p(ti),
                              tv.shape[-1] if tv is not None else 0, p(lengths), Bn, Tn, V, tau, p(gscale), p(loss), p(row_kl), p(dl), ldd,
                              p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.otr_last_error_string()
    torch.cuda.synchronize()
    return {'loss': loss.cpu().numpy(), 'row_kl': row_kl.cpu().numpy(), 'dlogits': dl.cpu().numpy() if grad else None}


def _check(tag, got, want, want32, V, tau, g=1.0):
    """the bounds of the module docstring; prints what was measured beside them"""
    live = want['live']
    d0_kl = float(np.abs(want32['row_kl'].astype(np.float64) - want['row_kl']).max())
    b_kl = 4 * max(d0_kl, 1e-6)
    e_kl = float(np.abs(got['row_kl'] - want['row_kl']).max())
    e_loss = abs(float(got['loss'][0]) - float(want['loss']))
    line = 'distill %s: |row_kl err| %.3g (d0 %.3g, bound %.3g), |loss err| %.3g (bound %.3g)' % (tag, e_kl, d0_kl, b_kl, e_loss, tau * tau * b_kl)
    assert np.all(got['row_kl'][~live] == 0)
    d = got['dlogits']
    if d is not None:
        d3 = d.reshape(B, T, -1)
        assert np.all(d3[:, :, V:] == 0)                      # the pad columns (a NaN would fail the comparison)
        assert np.all(d3[~live] == 0)                         # dead rows: exactly zero
        if want['n_live']:
            pq = (want['p'] + want['q'])[live]
            diff = (want['p'] - want['q'])[live]
            u32 = (want32['p'].astype(np.float64) - want32['q'].astype(np.float64))[live]
            d0_g = float((np.abs(u32 - diff) / pq).max())
            u = d3[:, :, :V][live].astype(np.float64) * want['n_live'] / (g * tau)
            e_g = float((np.abs(u - diff) / pq).max())
            b_g = 4 * max(d0_g, 2e-6)
            line += ', max |u - (p - q)| / (p + q) %.3g (d0 %.3g, bound %.3g)' % (e_g, d0_g, b_g)
            print(line)
            assert np.all(np.abs(u - diff) <= b_g * pq), line
            line = None
    if line:
        print(line)
    assert e_kl <= b_kl and e_loss <= tau * tau * b_kl, line


# ---------------------------------------------------------------- the kernel, dense
@pytest.mark.parametrize('which', ['plain', 'clamped'])
@pytest.mark.parametrize('tau', [0.5, 1.0, 2.0, 4.0])
@pytest.mark.parametrize('V,pad', sorted(PADS))
def test_kernel_matches_restatement(V, pad, tau, which):
    s, t, lengths, want, want32 = _case(V, pad, tau, which)
    pad_t, pad_d = PADS[(V, pad)]
    assert want['n_live'] == (10 if which == 'plain' else 8)
    assert want['row_kl'][want['live']].mean() >= 0.01        # the test cannot pass on a vanishing signal
    s_d, t_d, n_d = _view(s, V), _view(t, V), _dev(lengths)
    got = _run(s_d, V, n_d, tau, teacher=t_d, ldd=V + pad_d)
    _check('V=%d pad=%d tau=%g %s' % (V, pad, tau, which), got, want, want32, V, tau)
    if which == 'plain':
        again = _run(s_d, V, n_d, tau, teacher=t_d, ldd=V + pad_d)
        for k in got:
            assert np.array_equal(got[k], again[k]), k        # the same bits on every run
        fwd = _run(s_d, V, n_d, tau, teacher=t_d, grad=False)
        assert np.array_equal(fwd['loss'], got['loss']) and np.array_equal(fwd['row_kl'], got['row_kl'])
        scaled = _run(s_d, V, n_d, tau, teacher=t_d, ldd=V + pad_d, gscale=torch.tensor([3.0], device=DEV))
        np.testing.assert_allclose(scaled['dlogits'], 3.0 * got['dlogits'], rtol=1e-6, atol=0)
        assert np.array_equal(scaled['loss'], got['loss'])
        _check('V=%d pad=%d tau=%g g=3' % (V, pad, tau), scaled, want, want32, V, tau, g=3.0)


@pytest.mark.parametrize('V,pad', [(37, 0), (4233, 7)])
def test_no_live_row_and_teacher_equal_to_student(V, pad):
    tau = 2.0
    s, t, lengths, want, _ = _case(V, pad, tau, 'plain')
    s_d, t_d = _view(s, V), _view(t, V)
    none = _run(s_d, V, _dev(np.zeros(B, np.int32)), tau, teacher=t_d, ldd=V + pad)
    assert none['loss'][0] == 0 and not none['dlogits'].any() and not none['row_kl'].any()
    same = _run(s_d, V, _dev(lengths), tau, teacher=s_d, ldd=V)
    pq = 2 * want['p'][want['live']]
    u = same['dlogits'].reshape(B, T, V)[want['live']].astype(np.float64) * want['n_live'] / tau
    print('distill V=%d teacher = student: max row_kl %.3g, max |u| / (p + q) %.3g' % (V, np.abs(same['row_kl']).max(), (np.abs(u) / pq).max()))
    assert np.all(np.abs(same['row_kl']) <= 1e-6) and np.all(np.abs(u) <= 8e-6 * pq)


@pytest.mark.parametrize('shift', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)])
def test_base_pointers_off_a_16_byte_boundary(shift):
    """row strides that are multiples of 4 floats (4240) under a base that is not 16-byte aligned: student, teacher and gradient are
    judged one by one, each takes the scalar route on its own; the results are those of the aligned call bit for bit"""
    V, pad, tau = 4233, 7, 2.0
    s, t, lengths, want, want32 = _case(V, pad, tau, 'plain')
    ld, n_d = V + pad, _dev(lengths)

    def shifted(a, k):
        buf = torch.zeros(a.size + k, device=DEV)
        buf[k:] = _dev(a).reshape(-1)
        v = buf[k:].view(B, T, ld)[..., :V]
        assert (v.data_ptr() % 16 != 0) == (k != 0) and v.stride(1) % 4 == 0
        return v
    got = _run(shifted(s, shift[0]), V, n_d, tau, teacher=shifted(t, shift[1]), ldd=ld, dl_shift=shift[2])
    _check('V=%d shifts %s' % (V, (shift,)), got, want, want32, V, tau)
    base = _run(shifted(s, 0), V, n_d, tau, teacher=shifted(t, 0), ldd=ld)
    for k in got:
        assert np.array_equal(got[k], base[k]), k
    val, idx = ref.topk(t[:, :, :V], 40)
    top = (_dev(val), _dev(idx))
    sp = _run(shifted(s, shift[0]), V, n_d, tau, top=top, ldd=ld, dl_shift=shift[2])
    sp0 = _run(shifted(s, 0), V, n_d, tau, top=top, ldd=ld)
    for k in sp:
        assert np.array_equal(sp[k], sp0[k]), k


@pytest.mark.parametrize('V,pad', [(37, 0), (4233, 7)])
def test_teacher_entries_of_minus_infinity(V, pad):
    """a teacher element of -inf has q = 0 and a term of 0, never NaN; a teacher row of -inf throughout is dead"""
    tau = 2.0
    s, t, lengths, _, _ = _case(V, pad, tau, 'plain')
    t = t.copy()
    rng = np.random.default_rng(V)
    t[:, :, :V][rng.random((B, T, V)) < 0.3] = -np.inf
    t[0, 0, :V - 1] = -np.inf                                 # all the mass on one element
    t[0, 1, :V] = -np.inf                                     # no mass at all
    want = ref.forward(s, lengths, V, tau, teacher=t)
    want32 = ref.forward(s, lengths, V, tau, teacher=t, dtype=np.float32)
    assert want['n_live'] == 9 and not want['live'][0, 1] and np.isfinite(want['grad']).all()
    got = _run(_view(s, V), V, _dev(lengths), tau, teacher=_view(t, V), ldd=V + pad)
    assert np.isfinite(got['dlogits']).all() and np.isfinite(got['row_kl']).all()
    _check('V=%d -inf' % V, got, want, want32, V, tau)


# ---------------------------------------------------------------- the kernel, sparse
@pytest.mark.parametrize('V,pad,K,tau', [(100, 4, 1, 2.0), (100, 4, 8, 1.0), (100, 4, 40, 2.0), (4233, 7, 8, 2.0), (4233, 7, 40, 0.5),
                                         (4233, 7, 128, 2.0), (4234, 6, 40, 4.0), (8192, 3, 128, 1.0)])
def test_sparse_kernel_matches_restatement(V, pad, K, tau):
    s, t, lengths, _, _ = _case(V, pad, tau, 'plain')
    val, idx = ref.topk(t[:, :, :V], K)
    want = ref.forward(s, lengths, V, tau, top_val=val, top_idx=idx)
    want32 = ref.forward(s, lengths, V, tau, top_val=val, top_idx=idx, dtype=np.float32)
    if K > 1:
        assert want['row_kl'][want['live']].mean() >= 0.01
    _, pad_d = PADS[(V, pad)]
    s_d, n_d, top = _view(s, V), _dev(lengths), (_dev(val), _dev(idx))
    got = _run(s_d, V, n_d, tau, top=top, ldd=V + pad_d)
    _check('V=%d pad=%d K=%d tau=%g' % (V, pad, K, tau), got, want, want32, V, tau)
    again = _run(s_d, V, n_d, tau, top=top, ldd=V + pad_d)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    fwd = _run(s_d, V, n_d, tau, top=top, grad=False)
    assert np.array_equal(fwd['loss'], got['loss']) and np.array_equal(fwd['row_kl'], got['row_kl'])


def test_sparse_indices_out_of_range_and_an_empty_row():
    """V = 5 with K = 8: indices outside [0, V) on both sides drop their entries and are never used as addresses; a row without a
    valid entry is dead"""
    V, K, tau = 5, 8, 1.0
    s, _, _, _, _ = _case(V, 0, tau, 'plain')
    rng = np.random.default_rng(11)
    lengths = np.array([7, 7, 7], np.int32)
    val = rng.normal(size=(B, T, K)).astype(np.float32) * 3
    idx = np.tile(np.array([0, -1, 1, V, 2, 1 << 30, 3, -(1 << 31)], np.int64), (B, T, 1)).astype(np.int32)
    idx[0, 2] = [-1, V, V + 1, -7, 99, 1 << 20, -(1 << 31), V]
    idx[2, 5] = [4, 3, 2, 1, 0, -1, V, 1 << 30]
    want = ref.forward(s, lengths, V, tau, top_val=val, top_idx=idx)
    want32 = ref.forward(s, lengths, V, tau, top_val=val, top_idx=idx, dtype=np.float32)
    assert want['n_live'] == 20 and not want['live'][0, 2]
    got = _run(_dev(s), V, _dev(lengths), tau, top=(_dev(val), _dev(idx)))
    _check('V=5 K=8 out-of-range', got, want, want32, V, tau)


def test_topk_rows_then_sparse_op_is_the_dense_op_at_full_width():
    """ops.topk_rows with K = V = 100 lists the whole row: ops.distill_loss_topk on it agrees with the dense restatement, and with
    ops.distill_loss on the same tensors, within the dense bounds; rows past lengths come back as zeros"""
    from opentransformer_amd import ops
    V, pad, tau = 100, 4, 2.0
    s, t, lengths, want, want32 = _case(V, pad, tau, 'plain')
    s_d, t_d, n_d = _view(s, V), _view(t, V), _dev(lengths)
    val, idx = ops.topk_rows(t_d, n_d, V)
    assert val.shape == (B, T, V) and idx.dtype == torch.int32
    rv, ri = ref.topk(t[:, :, :V], V)
    live = want['live']
    assert np.array_equal(val.cpu().numpy()[live], rv[live]) and np.array_equal(idx.cpu().numpy()[live], ri[live])
    assert not val.cpu().numpy()[~live].any() and not idx.cpu().numpy()[~live].any()
    leaf = s_d.clone().requires_grad_(True)
    loss, row_kl = ops.distill_loss_topk(leaf, val, idx, n_d, temperature=tau)
    ops.backward(loss)
    torch.cuda.synchronize()
    got = {'loss': loss.detach().reshape(1).cpu().numpy(), 'row_kl': row_kl.cpu().numpy(), 'dlogits': leaf.grad.reshape(B * T, V).cpu().numpy()}
    _check('topk_rows K=V=100', got, want, want32, V, tau)
    # the sparse op against the dense OP under the same bounds: row_kl, loss, and the gradients relative to p + q
    leaf2 = s_d.clone().requires_grad_(True)
    dense_loss, dense_kl = ops.distill_loss(leaf2, t_d, n_d, temperature=tau)
    ops.backward(dense_loss)
    torch.cuda.synchronize()
    b_kl = 4 * max(float(np.abs(want32['row_kl'].astype(np.float64) - want['row_kl']).max()), 1e-6)
    pq = want['p'] + want['q']
    b_g = 4 * max(float((np.abs((want32['p'].astype(np.float64) - want32['q']) - (want['p'] - want['q']))[live] / pq[live]).max()), 2e-6)
    scale = want['n_live'] / tau
    du = np.abs(leaf.grad.cpu().numpy().astype(np.float64) - leaf2.grad.cpu().numpy()) * scale
    e_kl = float(np.abs(row_kl.cpu().numpy() - dense_kl.cpu().numpy()).max())
    print('distill topk_rows K=V=100 against the dense op: |row_kl diff| %.3g (bound %.3g), |loss diff| %.3g (bound %.3g), '
          'max |u diff| / (p + q) %.3g (bound %.3g)' % (e_kl, b_kl, abs(loss.item() - dense_loss.item()), tau * tau * b_kl,
                                                      float((du[live] / pq[live]).max()), b_g))
    assert e_kl <= b_kl and abs(loss.item() - dense_loss.item()) <= tau * tau * b_kl
    assert np.all(du[live] <= b_g * pq[live]) and not du[~live].any()
    assert not row_kl.requires_grad and not dense_kl.requires_grad


# ---------------------------------------------------------------- ops.distill_loss through autograd
def test_op_gradient_through_a_row_padded_view():
    """ops.distill_loss on the [B, T, V] head of a [R, V8] product: the gradient of the padded leaf is the kernel's, zero in the tail,
    and a seed other than ops.backward's unit scalar multiplies it"""
    from opentransformer_amd import ops
    V, pad, tau = 4234, 6, 2.0
    s, t, lengths, _, _ = _case(V, pad, tau, 'plain')
    n_d, t_d = _dev(lengths), _view(t, V)
    direct = _run(_view(s, V), V, n_d, tau, teacher=t_d, ldd=V + pad)
    full = _dev(s).reshape(B * T, V + pad).requires_grad_(True)
    loss, row_kl = ops.distill_loss(full[:, :V].view(B, T, V), t_d, n_d, temperature=tau)
    assert not row_kl.requires_grad and row_kl.shape == (B, T)
    ops.backward(loss)
    torch.cuda.synchronize()
    assert loss.item() == float(direct['loss'][0])
    assert np.array_equal(full.grad.cpu().numpy(), direct['dlogits'])
    assert np.array_equal(row_kl.cpu().numpy(), direct['row_kl'])
    full2 = _dev(s).reshape(B * T, V + pad).requires_grad_(True)
    loss2, _ = ops.distill_loss(full2[:, :V].view(B, T, V), t_d, n_d, temperature=tau)
    (loss2 * 3.0).backward()
    np.testing.assert_allclose(full2.grad.cpu().numpy(), 3.0 * direct['dlogits'], rtol=1e-6, atol=0)
    full3 = _dev(s).reshape(B * T, V + pad).requires_grad_(True)
    loss3, _ = ops.distill_loss(full3[:, :V].view(B, T, V), t_d, n_d, temperature=tau, grad_scale=torch.tensor(3.0, device=DEV))
    ops.backward(loss3)
    np.testing.assert_allclose(full3.grad.cpu().numpy(), 3.0 * direct['dlogits'], rtol=1e-6, atol=0)
    with torch.no_grad():                                   # no gradient wanted: forward only
        loss4, _ = ops.distill_loss(full[:, :V].view(B, T, V), t_d, n_d, temperature=tau)
    assert loss4.item() == loss.item() and not loss4.requires_grad
    t_leaf = t_d.clone().requires_grad_(True)               # the teacher takes no gradient
    loss5, _ = ops.distill_loss(_view(s, V), t_leaf, n_d, temperature=tau)
    assert not loss5.requires_grad


# ---------------------------------------------------------------- model level
TAU = 2.0


def _model_case(mode, kind):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ops.set_compute_dtype(mode)
    cfg = syn.c1_model(0.0, ctc_weight=0.3 if kind == 'joint' else 0.0)
    if kind == 'ctc':
        cfg = dict(cfg, vocab_size=cfg['decoder']['vocab_size'])
    cls = ota.CTCModel if kind == 'ctc' else ota.SpeechToText
    pair = []
    for seed in (1234, 4321):                               # student, teacher: the same architecture, different weights
        m = cls(cfg)
        syn.fill_state_dict_(m.state_dict(), seed)
        pair.append(m.to(DEV))
    V = cfg['decoder']['vocab_size']
    inputs, targets = syn.synthetic_batch(4, 96, 80, V, 6, seed=5, lengths=[96, 80, 96, 64], tgt_lengths=[6, 4, 5, 6])
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    return pair[0].train(), pair[1], inputs, targets


def _kd_torch(logits, teacher, lengths, dtype):
    """tau^2 / n_live * sum over the live rows of KL(softmax(teacher / tau) || softmax(logits / tau)) from torch ops in `dtype`"""
    lp = torch.log_softmax(logits.to(dtype) / TAU, dim=-1)
    lq = torch.log_softmax(teacher.to(dtype) / TAU, dim=-1)
    live = torch.arange(logits.shape[1], device=logits.device).unsqueeze(0) < lengths.clamp(0, logits.shape[1]).unsqueeze(1)
    kl = (lq.exp() * (lq - lp)).sum(-1)
    return TAU * TAU * torch.where(live, kl, torch.zeros_like(kl)).sum() / live.sum()


def _student_logits(model, inputs, targets):
    """the student's forward as DistillTraining runs it: (own loss, {head: (logits, lengths)}, CTC weight)"""
    import opentransformer_amd as ota
    truth, truth_length = targets['targets'], targets['targets_length']
    x, mask = model.frontend(inputs['inputs'], inputs['mask'])
    memory, memory_mask, _ = model.encoder(x, mask)
    memory_length = torch.sum(memory_mask, dim=-1)
    if isinstance(model, ota.CTCModel):
        ctc = model.assistor(memory, return_logits=True)
        own = model.assistor.compute_loss(ctc, memory_length, truth[:, 1:-1].contiguous(), truth_length.add(-1))
        return own, {'ctc': (ctc, memory_length)}, 1.0
    logits, _ = model.decoder(truth[:, :-1], memory, memory_mask)
    own = model.crit(logits, truth[:, 1:])
    heads = {'att': (logits, truth_length)}
    if model.ctc_weight > 0:
        ctc = model.assistor(memory, return_logits=True)
        own = (1 - model.ctc_weight) * own + model.ctc_weight * model.assistor.compute_loss(ctc, memory_length, truth[:, 1:].contiguous(), truth_length)
        heads['ctc'] = (ctc, memory_length)
    return own, heads, float(model.ctc_weight)


def _composed_step(model, inputs, targets, teacher_out, kd_weight, dtype):
    """DistillTraining.forward with the distillation term (and only it) composed from torch ops in `dtype` on the model's own logits"""
    own, heads, w = _student_logits(model, inputs, targets)
    kds = {k: _kd_torch(lg, teacher_out[k], n, dtype) for k, (lg, n) in heads.items()}
    kd = (1 - w) * kds['att'] + w * kds['ctc'] if len(kds) == 2 else next(iter(kds.values()))
    return (1 - kd_weight) * own + kd_weight * kd.float(), kd, kds


def _grads(model, loss):
    from opentransformer_amd import ops
    for p in model.parameters():
        p.grad = None
    ops.backward(loss)
    torch.cuda.synchronize()
    named = [(n, p.grad.detach().clone()) for n, p in model.named_parameters() if p.grad is not None]
    return [n for n, _ in named], [g for _, g in named]


@pytest.mark.parametrize('kind', ['att', 'joint', 'ctc'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_training_step_matches_the_composed_loss(mode, kind):
    """DistillTraining.forward + ops.backward against the same model with the distillation term composed from torch ops in float64 on
    the same logits.  Loss: the kernel bound, tau^2 4 max(d0, 1e-6) with d0 the distance of the float32 composition from the float64
    one; the total loss: kd_weight times that, plus, where the student has a CTC head, 4 * 2^-23 of the larger of the loss and
    the CTC term -- its own loss is recomputed by the composed route, and otr_ctc_loss adds its B = 4 terms with floating-point
    atomics, so two passes differ in the order of those additions (see test_kd_weight_zero_is_the_plain_step).  Parameter gradients (tests.helpers.key_aware_grad_errors): max(1e-4, 4 d0) as in tests/test_gpu_mwer.py, d0 the distance
    between the composed route with float32 and with float64 loss math."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, teacher, inputs, targets = _model_case(mode, kind)
        before = {k: v.clone() for k, v in teacher.state_dict().items()}
        fault = ops.fault_counter(torch.device(DEV, torch.cuda.current_device()))
        fault.zero_()
        kd_weight = 0.5
        wrap = ota.DistillTraining(model, teacher, kd_weight=kd_weight, temperature=TAU)
        assert model.training and not teacher.training and wrap.model is model
        loss, aux = wrap(inputs, targets)
        names, got = _grads(model, loss)
        teacher_out = wrap.teacher_outputs(inputs, targets)
        assert sorted(teacher_out) == {'att': ['att'], 'joint': ['att', 'ctc'], 'ctc': ['ctc']}[kind]
        total64, kd64, kds64 = _composed_step(model, inputs, targets, teacher_out, kd_weight, torch.float64)
        names64, want = _grads(model, total64)
        total32, kd32, _ = _composed_step(model, inputs, targets, teacher_out, kd_weight, torch.float32)
        _, base = _grads(model, total32)
        assert names == names64 and len(names) > 10
        assert sorted(aux) == sorted(['Loss', 'KD', 'KD_att', 'KD_ctc'] + (['CTCLoss'] if kind != 'att' else []))
        assert kd64.item() >= 0.01                          # two models with different weights: the signal does not vanish
        bound = TAU * TAU * 4 * max(abs(float(kd32) - float(kd64)) / (TAU * TAU), 1e-6)
        print('distill model %s %s: KD %.7f composed %.7f (bound %.3g), total %.7f composed %.7f' % (
            mode, kind, float(aux['KD']), float(kd64), bound, loss.item(), total64.item()))
        assert abs(float(aux['KD']) - float(kd64)) <= bound
        for k, v in kds64.items():
            assert abs(float(aux['KD_' + k]) - float(v)) <= bound, k
        slack = 4 * 2.0 ** -23 * max(abs(total64.item()), float(aux['CTCLoss'])) if kind != 'att' else 0.0
        assert abs(loss.item() - total64.item()) <= kd_weight * bound + slack
        d_model = 64                                        # syn.c1_model
        errs, key_errs = H.key_aware_grad_errors(names, got, want, d_model)
        d0, _ = H.key_aware_grad_errors(names, base, want, d_model)
        worst = max(errs, key=lambda k: errs[k] / max(1e-4, 4 * d0[k]))
        print('  grads: worst %s err %.3g bound %.3g; max err %.3g, max d0 %.3g, max key residue %.3g' % (
            worst, errs[worst], max(1e-4, 4 * d0[worst]), max(errs.values()), max(d0.values()), max(key_errs.values(), default=0.0)))
        assert len(errs) > 10
        for k, e in errs.items():
            assert e <= max(1e-4, 4 * d0[k]), (k, e, d0[k])
        # the teacher is nobody's parameter: a backward pass and an optimizer step leave it as it was
        opt = torch.optim.SGD(wrap.parameters(), lr=0.1)
        opt.step()
        torch.cuda.synchronize()
        for k, v in teacher.state_dict().items():
            assert torch.equal(v, before[k]), k
        assert all(p.grad is None for p in teacher.parameters())
        assert int(fault.item()) == 0
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('kind', ['att', 'joint', 'ctc'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_kd_weight_zero_is_the_plain_step(mode, kind):
    """kd_weight = 0: the step's loss is the student's own loss bit for bit, and its gradients are the plain step's to 1e-6 relative.
    Against a separate plain forward pass the loss is equal bit for bit where that pass is reproducible (no CTC head).  otr_ctc_loss
    adds the utterances' terms into the mean with floating-point atomics, so two plain passes of a model with a CTC head differ from
    each other in the order of B = 4 additions: at most (B - 1) roundings of 2^-24 relative each way, 4 * 2^-23 covers it."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, teacher, inputs, targets = _model_case(mode, kind)
        plain, _ = model(inputs, targets)
        names0, want = _grads(model, plain)
        loss, aux = ota.DistillTraining(model, teacher, kd_weight=0.0, temperature=TAU)(inputs, targets)
        names, got = _grads(model, loss)
        assert loss.item() == float(aux['Loss']) and float(aux['KD']) > 0.01
        print('distill kd_weight=0 %s %s: loss %.9g plain %.9g' % (mode, kind, loss.item(), plain.item()))
        assert abs(loss.item() - plain.item()) <= (0.0 if kind == 'att' else 4 * 2.0 ** -23 * abs(plain.item()))
        assert names == names0 and len(names) > 10
        errs, _ = H.key_aware_grad_errors(names, got, want, 64)
        print('distill kd_weight=0 %s %s: max relative gradient error %.3g' % (mode, kind, max(errs.values())))
        assert max(errs.values()) <= 1e-6, max(errs, key=errs.get)
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('kind', ['att', 'joint', 'ctc'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_teacher_copy_offline_outputs_and_topk(mode, kind):
    """a teacher that is a copy of the student gives KD <= 1e-6; teacher_outputs() fed back as teacher_out is the online step (and needs
    no teacher): the distillation terms bit for bit, and so the whole loss where the student's own loss is reproducible -- with a CTC
    head it is not, otr_ctc_loss adds its B = 4 terms with floating-point atomics (see test_kd_weight_zero_is_the_plain_step), there
    the two losses agree to 4 * 2^-23 of the larger of the loss and the CTC term; with topk = K the step's terms are
    ops.distill_loss_topk on the same pairs"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, teacher, inputs, targets = _model_case(mode, kind)
        heads = {'att': ['att'], 'joint': ['att', 'ctc'], 'ctc': ['ctc']}[kind]
        model.eval()                                        # (no dropout in this model: eval() only makes the copy comparison literal)
        twin = ota.DistillTraining(model, copy.deepcopy(model), temperature=TAU)
        _, aux = twin(inputs, targets)
        print('distill %s %s: KD against a copy of the student %.3g' % (mode, kind, float(aux['KD'])))
        assert abs(float(aux['KD'])) <= 1e-6 and abs(float(aux['KD_att'])) <= 1e-6 and abs(float(aux['KD_ctc'])) <= 1e-6

        def same_loss(a, b, aux_a):
            slack = 4 * 2.0 ** -23 * max(abs(a.item()), float(aux_a['CTCLoss'])) if kind != 'att' else 0.0
            return abs(a.item() - b.item()) <= slack
        model.train()
        wrap = ota.DistillTraining(model, teacher, temperature=TAU)
        online, aux_on = wrap(inputs, targets)
        stored = wrap.teacher_outputs(inputs, targets)
        offline, aux_off = ota.DistillTraining(model, None, temperature=TAU)(inputs, targets, teacher_out=stored)
        assert same_loss(online, offline, aux_on) and all(torch.equal(aux_on[k], aux_off[k]) for k in ('KD', 'KD_att', 'KD_ctc'))
        assert sorted(stored) == heads and (float(aux_on['KD_ctc']) > 0.01) == (kind != 'att')
        K = 40
        sparse = ota.DistillTraining(model, teacher, temperature=TAU, topk=K)
        pairs = sparse.teacher_outputs(inputs, targets)
        assert sorted(pairs) == heads and all(pairs[k][0].shape[-1] == K and pairs[k][1].dtype == torch.int32 for k in heads)
        loss_k, aux_k = sparse(inputs, targets)
        loss_k2, aux_k2 = ota.DistillTraining(model, None, temperature=TAU)(inputs, targets, teacher_out=pairs)
        assert same_loss(loss_k, loss_k2, aux_k) and all(torch.equal(aux_k[k], aux_k2[k]) for k in ('KD', 'KD_att', 'KD_ctc'))
        for k, (lg, n) in _student_logits(model, inputs, targets)[1].items():
            direct, _ = ops.distill_loss_topk(lg, pairs[k][0], pairs[k][1], n, temperature=TAU)
            assert direct.item() == float(aux_k['KD_' + k]), k
        assert float(aux_k['KD']) != float(aux_on['KD']) and float(aux_k['KD']) > 0.01
        with pytest.raises(ValueError, match='teacher'):
            ota.DistillTraining(model, None)(inputs, targets)
        short = {k: v[:, :-1] for k, v in stored.items()}
        with pytest.raises(ValueError, match='teacher has'):   # a teacher with another subsampling / target length
            ota.DistillTraining(model, None)(inputs, targets, teacher_out=short)
    finally:
        ops.set_compute_dtype('bf16')
