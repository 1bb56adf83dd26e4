"""GPU (-m gpu): the transducer's kernels (csrc/rnnt.hip), wrappers, model and greedy recognizer against the float64 restatement of
tests/rnnt_ref.py on the CPU, on the cases of tests/rnnt_cases.py (checked on the CPU by tests/test_rnnt.py).

The loss is judged per utterance and per case: err_b <= K * floor_b + tiny_b for nll_b and for the gradient slab (relative Frobenius
norm), floor_b the distance of the restatement run in float32 from the same in float64, tiny_b = (T_b + U_b) * eps_fp32 * max |lp_b|
(rnnt_cases.floor_of).  The sum of every live gradient row stays under the same bound relative to max(the row's absolute sum, the
row's occupancy): a row is p * occupancy minus two terms that add up to the occupancy, so where the softmax is saturated (`peaked`)
the row itself is orders of magnitude smaller than the terms it is the difference of, and the restatement's own float64 rows then
sum to zero only relative to those terms (tests/test_rnnt.py holds it to 1e-12 of that).  Every test writes what it measured into
parity_out/rnnt_parity.json (or under $OTR_PARITY_DIR) before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import helpers as H
from tests import rnnt_cases as rc
from tests import rnnt_ref as rr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# err_b <= K * floor_b + tiny_b.  Measured on MI355X (profiles/rnnt_parity.json), over all cases, utterances and both call paths.
# The lattice kernel sweeps on shifted log-probs lp + c (include/otrans_hip.h), so alpha, beta and the exponents of the gradient are
# small numbers whatever the lattice's size, and the gradient slab no longer leans on tiny_b: its worst err / floor is 3.71
# (wave_edges, U_b 255: 3.3e-5 against 8.9e-6; long_t, T_b 299: 1.38; every slab is at most 0.14 x tiny_b).  K_MEASURED is that
# ratio and K twice it, rounded up.  Three ratios are larger and are NOT what K is twice of, because there tiny_b, not the floor, is
# the yardstick: utterance 1 of `peaked` (gradient 67, row sums 85: max |lp| is 119 there, so float32 holds lp itself only to
# eps * 119 = 1.4e-5 absolute, which is what tiny_b = 1.1e-4 states; the error is 4.0e-6 against a floor of 5.9e-8), nll of
# vocab_4233 utterance 1 (12.1: the float32 restatement landed within a tenth of an ulp of float64, floor 6.1e-9, error 7.4e-8 =
# 0.6 ulp) and the row sums of the short cases (up to 6.3 x the GRADIENT's floor of 3e-8 .. 1.5e-7, a few eps in absolute terms).
K_MEASURED = 3.71
K = 8.0
REPORT = {}


def _report(name, tag, rec):
    REPORT.setdefault(name, {})[tag] = rec
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'rnnt_parity.json'), 'w') as f:
        json.dump(json.loads(json.dumps({'K': K, 'K_measured_worst_ratio': K_MEASURED, 'cases': REPORT}),
                             parse_float=lambda x: float('%.3g' % float(x))), f, sort_keys=True, indent=None, separators=(',', ':'))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _wide_labels(c, wide):
    """the labels as the [:, 1:-1]-like view of a matrix `wide` columns wider whose other columns hold a different valid label"""
    lab = c['labels']
    B, W = lab.shape
    V = c['logits'].shape[-1]
    big = torch.full((B, W + wide), 1 + int(lab[0, 0]) % (V - 1), dtype=torch.int64)
    big[big == lab[0, 0]] = 1 + (int(lab[0, 0]) + 1) % (V - 1)
    big[:, 1:1 + W] = lab
    big = big.to(DEV)
    view = big[:, 1:1 + W]
    assert view.stride(0) == W + wide and view.stride(1) == 1
    return view


def run_op(c, logits=None, wide=0):
    """ops.rnnt_loss as the model calls it: (loss, nll, valid, d loss / d logits) on the device"""
    from opentransformer_amd import ops
    x = (c['logits'] if logits is None else logits).to(DEV).requires_grad_(True)
    labels = _wide_labels(c, wide) if wide else c['labels'].to(DEV)
    loss, stats = ops.rnnt_loss(x, c['enc_len'].to(DEV), labels, c['tgt_len'].to(DEV))
    (g,) = torch.autograd.grad(loss, x)
    torch.cuda.synchronize()
    return loss.detach(), stats['nll'], stats['valid'], g


def run_direct(c, wide=0):
    """otr_rnnt_loss itself; the workspace, nll, valid and dlogits start as NaN / -7"""
    from opentransformer_amd import _lib as L
    B, T, U1, V = c['logits'].shape
    x = c['logits'].to(DEV).contiguous()
    labels = _wide_labels(c, wide) if wide else c['labels'].to(DEV).contiguous()
    el, tl = c['enc_len'].to(DEV), c['tgt_len'].to(DEV)
    lib = L.load()
    nws = lib.otr_rnnt_workspace_floats(B, T, U1)
    assert nws == 5 * B * T * U1 + 2 * B
    ws = torch.full((nws,), float('nan'), dtype=torch.float32, device=DEV)
    nll = torch.full((B,), float('nan'), dtype=torch.float32, device=DEV)
    loss = torch.full((), float('nan'), dtype=torch.float32, device=DEV)
    valid = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    dl = torch.full((B, T, U1, V), float('nan'), dtype=torch.float32, device=DEV)
    L.check(lib.otr_rnnt_loss(_p(x), V, _p(labels), labels.stride(0), _p(el), _p(tl), B, T, U1, V, 0, None, _p(loss), _p(nll), _p(valid),
                              _p(dl), V, _p(ws), nws, _stream()), 'otr_rnnt_loss')
    torch.cuda.synchronize()
    return loss, nll, valid, dl


def check_against_reference(name, tag, loss, nll, valid, g):
    c = rc.build(name)
    B, T, U1, V = c['logits'].shape
    ref_loss, ref_nll, ref_valid, ref_g = rc.reference_of(name)
    fl = rc.floor_of(name)
    _, occ = rc.closed_form_of(name)
    g, nll, valid = g.detach().cpu(), nll.cpu(), valid.cpu()
    e_grad = rc.slab_rel(g, ref_g)
    e_nll = (nll.double() - ref_nll).abs() / ref_nll.abs().clamp_min(1e-300)
    tiny_nll = fl['tiny'] / ref_nll.abs().clamp_min(1e-300)
    e_rows = rc.rowsum_rel(g, occ).reshape(B, -1).max(dim=1).values
    e_loss = abs(float(loss) - float(ref_loss)) / max(abs(float(ref_loss)), 1e-300)

    def ratios(e, f):
        return [float(e[b] / f[b]) if float(f[b]) > 0 and bool(ref_valid[b]) else None for b in range(B)]

    rec = {'shape': [B, T, U1, V], 'enc_len': c['enc_len'].tolist(), 'tgt_len': c['tgt_len'].tolist(), 'loss_err': e_loss,
           'grad_err': e_grad.tolist(), 'grad_floor': fl['grad'].tolist(), 'tiny': fl['tiny'].tolist(),
           'grad_err_over_floor': ratios(e_grad, fl['grad']), 'nll_err': e_nll.tolist(), 'nll_floor': fl['nll'].tolist(),
           'nll_tiny': tiny_nll.tolist(), 'nll_err_over_floor': ratios(e_nll, fl['nll']), 'rowsum_err': e_rows.tolist(),
           'rowsum_err_over_grad_floor': ratios(e_rows, fl['grad'])}
    for k in ('grad_err_over_floor', 'nll_err_over_floor', 'rowsum_err_over_grad_floor'):
        r = [x for x in rec[k] if x is not None]
        rec['max_' + k] = max(r) if r else None
    _report(name, tag, rec)
    print(name, tag, json.dumps({k: v for k, v in rec.items() if k.startswith('max_') or k == 'loss_err'}))

    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(nll).all()) and bool(torch.isfinite(loss.cpu())), (name, tag)
    assert valid.tolist() == [int(v) for v in ref_valid.tolist()], (name, tag, valid.tolist())
    for b in range(B):
        Tb, Ub = int(c['enc_len'][b]), int(c['tgt_len'][b])
        where = (name, tag, 'utterance %d' % b, 'T_b %d' % Tb, 'U_b %d' % Ub)
        if not bool(ref_valid[b]):                                               # guarded: nll 0, valid 0, the whole slab zero
            assert float(g[b].abs().max()) == 0.0 and float(nll[b]) == 0.0, where + ('guarded',)
            continue
        dead = g[b].clone()
        dead[:Tb, :Ub + 1] = 0
        assert float(dead.abs().max()) == 0.0, where + ('rows outside the lengths',)
        # no live row is identically zero -- where float32 can hold it: a row whose largest float64 entry is below 1e-30 (`peaked`
        # has rows of 1e-89) may underflow to zero in float32, on the device as in the float32 run of the restatement
        top, top_ref = g[b, :Tb, :Ub + 1].abs().amax(-1), ref_g[b, :Tb, :Ub + 1].abs().amax(-1)
        assert bool((top[top_ref > 1e-30] > 0).all()), where + ('a live row is identically zero',)
        assert float(e_nll[b]) <= K * float(fl['nll'][b]) + float(tiny_nll[b]), \
            where + ('nll', float(nll[b]), float(ref_nll[b]), float(e_nll[b]), float(fl['nll'][b]), float(tiny_nll[b]))
        if not float(e_grad[b]) <= K * float(fl['grad'][b]) + float(fl['tiny'][b]):
            per = (g[b].double() - ref_g[b]).norm(dim=-1)
            t, u = divmod(int(per.argmax()), U1)
            v = int((g[b, t, u].double() - ref_g[b, t, u]).abs().argmax())
            raise AssertionError(where + ('gradient slab', float(e_grad[b]), 'floor', float(fl['grad'][b]), 'tiny', float(fl['tiny'][b]),
                                          'worst row (%d, %d) column %d: got %.6e want %.6e' % (t, u, v, float(g[b, t, u, v]), float(ref_g[b, t, u, v]))))
        assert float(e_rows[b]) <= K * float(fl['grad'][b]) + float(fl['tiny'][b]), \
            where + ('row sums', float(e_rows[b]), float(fl['grad'][b]), float(fl['tiny'][b]))
    assert e_loss <= K * float(fl['nll'].max()) + float(tiny_nll.max()) if bool(ref_valid.any()) else float(loss) == 0.0, (name, tag, e_loss)


# ---------------------------------------------------------------------------------------------- 1. the loss kernel
@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_rnnt_loss_op_matches_float64_per_utterance(name):
    check_against_reference(name, 'op', *run_op(rc.build(name)))


@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_rnnt_loss_entry_matches_float64_per_utterance_from_poisoned_buffers(name):
    check_against_reference(name, 'direct', *run_direct(rc.build(name)))


def test_rnnt_loss_forward_only_leaves_no_gradient_and_the_same_numbers():
    from opentransformer_amd import ops
    c = rc.build('ragged')
    loss, nll, valid, _ = run_op(c)
    with torch.no_grad():
        loss2, stats = ops.rnnt_loss(c['logits'].to(DEV), c['enc_len'].to(DEV), c['labels'].to(DEV), c['tgt_len'].to(DEV))
    assert torch.equal(loss, loss2) and torch.equal(nll, stats['nll']) and torch.equal(valid, stats['valid']) and not loss2.requires_grad


def test_rnnt_loss_grad_scale_rides_in_the_gradient():
    from opentransformer_amd import ops
    c = rc.build('tiny')
    _, _, _, g1 = run_op(c)
    x = c['logits'].to(DEV).requires_grad_(True)
    loss, _ = ops.rnnt_loss(x, c['enc_len'].to(DEV), c['labels'].to(DEV), c['tgt_len'].to(DEV), grad_scale=torch.full((1,), 256.0, device=DEV))
    (g,) = torch.autograd.grad(loss, x)
    assert torch.equal(g, g1 * 256.0)                    # a power of two: exact


# ---------------------------------------------------------------------------------------------- 2. poison
def test_rnnt_loss_ignores_everything_outside_the_lengths():
    c = rc.build('ragged')
    loss, nll, valid, g = run_op(c)
    bad = c['logits'].clone()
    for b in range(bad.shape[0]):
        Tb, Ub = int(c['enc_len'][b]), int(c['tgt_len'][b])
        m = torch.ones(bad.shape[1:3], dtype=torch.bool)
        m[:Tb, :Ub + 1] = False
        bad[b][m] = float('nan')
        bad[b][m & (torch.arange(bad.shape[2]) % 2 == 0)] = float('inf')
    assert int(torch.isnan(bad).sum()) > 0 and int(torch.isinf(bad).sum()) > 0
    loss2, nll2, valid2, g2 = run_op(c, logits=bad)
    _report('ragged', 'poison', {'bit_equal': [bool(torch.equal(loss, loss2)), bool(torch.equal(nll, nll2)), bool(torch.equal(g, g2))]})
    assert torch.equal(loss, loss2) and torch.equal(nll, nll2) and torch.equal(valid, valid2) and torch.equal(g, g2)


# ---------------------------------------------------------------------------------------------- 3. label stride
@pytest.mark.parametrize('name', ['ragged', 'guarded'])
def test_rnnt_loss_reads_a_strided_label_view_in_place(name):
    c = rc.build(name)
    for tag, run in (('op', run_op), ('direct', run_direct)):
        loss, nll, valid, g = run(c)
        loss2, nll2, valid2, g2 = run(c, wide=3)
        _report(name, 'stride_' + tag, {'bit_equal': [bool(torch.equal(loss, loss2)), bool(torch.equal(nll, nll2)), bool(torch.equal(g, g2))]})
        assert torch.equal(loss, loss2) and torch.equal(nll, nll2) and torch.equal(valid, valid2) and torch.equal(g, g2), (name, tag)


# ---------------------------------------------------------------------------------------------- 4. the joint
JOINT_SHAPES = {'J4': (3, 7, 5, 4, [7, 4, 1], [4, 0, 2]), 'J64': (3, 7, 5, 64, [7, 4, 1], [4, 0, 2]), 'J260': (3, 7, 5, 260, [7, 4, 1], [4, 0, 2]),
                'U256': (2, 2, 256, 8, [2, 1], [255, 100])}


def _joint_inputs(key):
    B, T, U1, J, el, tl = JOINT_SHAPES[key]
    g = torch.Generator().manual_seed(40 + J + U1)
    pe, pg, dz = (torch.randn(s, generator=g) for s in ((B, T, J), (B, U1, J), (B, T, U1, J)))
    el, tl = torch.tensor(el, dtype=torch.int32), torch.tensor(tl, dtype=torch.int32)
    live = torch.zeros((B, T, U1), dtype=torch.bool)
    for b in range(B):
        live[b, :int(el[b]), :int(tl[b]) + 1] = True
    return pe, pg, dz, el, tl, live


def _joint_reference(pe, pg, dz, el, tl, live, dtype):
    pe, pg = pe.to(dtype).requires_grad_(True), pg.to(dtype).requires_grad_(True)
    z = rr.joint_ref(pe, pg, el, tl)
    dpe, dpg = torch.autograd.grad(z, (pe, pg), torch.where(live[..., None], dz.to(dtype), torch.zeros((), dtype=dtype)))
    return z.detach(), dpe, dpg


def _joint_device(pe, pg, dz, el, tl, live):
    from opentransformer_amd import ops
    nan = torch.full((), float('nan'))
    pe_p = torch.where((torch.arange(pe.shape[1])[None, :] < el[:, None])[..., None], pe, nan)
    pg_p = torch.where((torch.arange(pg.shape[1])[None, :] <= tl[:, None])[..., None], pg, nan)
    dz_p = torch.where(live[..., None], dz, nan)
    pe_d, pg_d = pe_p.to(DEV).requires_grad_(True), pg_p.to(DEV).requires_grad_(True)
    z = ops.rnnt_joint(pe_d, pg_d, el.to(DEV), tl.to(DEV))
    dpe, dpg = torch.autograd.grad(z, (pe_d, pg_d), dz_p.to(DEV))
    torch.cuda.synchronize()
    return z.detach(), ops.lp_of(z), dpe, dpg


@pytest.mark.parametrize('key', sorted(JOINT_SHAPES))
def test_rnnt_joint_matches_float64_and_never_reads_outside_the_lengths(key):
    from opentransformer_amd import ops
    args = _joint_inputs(key)
    want = _joint_reference(*args, torch.float64)
    floor = [rel(a.numpy(), b.numpy()) for a, b in zip(_joint_reference(*args, torch.float32), want)]
    eps = float(torch.finfo(torch.float32).eps)
    rec, got32 = {'floor': floor}, None
    try:
        for mode in ('fp32', 'bf16', 'fp16'):
            ops.set_compute_dtype(mode)
            z, z16, dpe, dpg = _joint_device(*args)
            got = (z.cpu(), dpe.cpu(), dpg.cpu())
            err = [rel(a.numpy(), b.numpy()) for a, b in zip(got, want)]
            rec[mode] = {'err': err, 'err_over_floor': [e / f if f > 0 else None for e, f in zip(err, floor)]}
            _report('joint_' + key, 'joint', rec)
            assert all(bool(torch.isfinite(t).all()) for t in got), (key, mode)
            live = args[-1]
            assert float(got[0][~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, (key, mode)
            if mode == 'fp32':
                assert z16 is None
                got32 = got
                for e, f, what in zip(err, floor, ('z', 'dpe', 'dpg')):
                    assert e <= K * f + eps, (key, what, e, f)
            else:                                        # only the twin differs, and it is the rounded f32 z
                assert all(torch.equal(a, b) for a, b in zip(got, got32)), (key, mode)
                assert z16.dtype == ops.half_dtype() and torch.equal(z16.cpu(), got[0].to(ops.half_dtype())), (key, mode)
    finally:
        ops.set_compute_dtype('bf16')


# ---------------------------------------------------------------------------------------------- 5. the model
C1_BATCH = dict(batch=4, frames=200, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[200, 180, 150, 97], tgt_lengths=[10, 8, 10, 5])


def _oracle_memory(inputs, parts, cfg):
    from oracle import otrans_oracle as orc
    x, mask = orc.conv_frontend(parts['frontend'], inputs['inputs'], inputs['mask'])
    return orc.transformer_encoder(parts['encoder'], x, mask, cfg['encoder'])


def _load(model, parts, own):
    model.frontend.load_state_dict({k: v.detach() for k, v in parts['frontend'].items()}, strict=True)
    model.encoder.load_state_dict({k: v.detach() for k, v in parts['encoder'].items()}, strict=True)
    model.predictor.load_state_dict({k[len('predictor.'):]: v.detach().float() for k, v in own.items() if k.startswith('predictor.')}, strict=True)
    model.joint.load_state_dict({k[len('joint.'):]: v.detach().float() for k, v in own.items() if k.startswith('joint.')}, strict=True)
    return model


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_transducer_model_matches_cpu_oracle(mode):
    """TransducerModel on the C1 frontend and encoder against the oracle's frontend and encoder (float32 on the CPU) followed by
    torch.nn.Embedding / torch.nn.LSTM / three F.linear / rnnt_loss_ref in float64; the form and the bounds of
    test_gpu_model.test_ctc_model_matches_cpu_oracle"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    cfg = syn.c1_model(0.0)
    inputs, targets = syn.synthetic_batch(**C1_BATCH)
    parts = H.require_grad(H.filled_state(cfg, seed=21))
    own = {k: v.double().requires_grad_(True) for k, v in rr.transducer_weights(seed=22).items()}
    memory, mmask = _oracle_memory(inputs, parts, cfg)
    truth = targets['targets']
    logits = rr.TransducerRef(own).logits(memory.double(), truth[:, :-1])
    ref, ref_nll, ref_valid = rr.rnnt_loss_ref(logits, mmask.sum(-1), truth[:, 1:-1], targets['targets_length'] - 1)
    assert bool(ref_valid.all())
    ref.backward()
    ops.set_compute_dtype(mode)
    try:
        model = _load(ota.TransducerModel(rc.model_config()), parts, own).to(DEV).train()
        with H.loss_scaled(mode) as ls:
            loss, aux = model(to_dev(inputs), to_dev(targets))
            loss.backward()
            ls.unscale(model)
        torch.cuda.synchronize()
        assert aux is None
        flat = {'frontend.' + k: v for k, v in parts['frontend'].items()}
        flat.update({'encoder.' + k: v for k, v in parts['encoder'].items()})
        flat.update(own)
        errs = {k: rel(p.grad.cpu().numpy(), flat[k].grad.numpy()) for k, p in model.named_parameters()}
        e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
        _report('model', mode, {'loss': loss.item(), 'ref': ref.item(), 'loss_err': e_loss, 'worst_grad': max(errs.values()),
                                'worst_grad_key': max(errs, key=errs.get), 'grad_err': errs})
        print('model', mode, e_loss, max(errs, key=errs.get), max(errs.values()))
        assert e_loss < (1e-5 if mode == 'fp32' else 5e-4), (loss.item(), ref.item())
        assert sorted(errs) == sorted(flat)
        for k, e in errs.items():
            assert e < (2e-3 if mode == 'fp32' else 1e-2), (k, e)
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_one_fused_adam_step_changes_every_transducer_parameter(mode):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    cfg = syn.c1_model(0.0)
    inputs, targets = syn.synthetic_batch(**C1_BATCH)
    ops.set_compute_dtype(mode)
    try:
        model = _load(ota.TransducerModel(rc.model_config()), H.filled_state(cfg, seed=21), rr.transducer_weights(seed=22)).to(DEV).train()
        dp = FlatDataParallel(model)
        opt = FusedAdam(dp, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-6, clip_grad=5.0)
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        dp.zero_grad(next_dropout_step=True)
        loss, _ = dp(to_dev(inputs), to_dev(targets))
        ops.backward(loss)
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        same = [k for k, p in model.named_parameters() if torch.equal(p.detach(), before[k])]
        _report('model', 'adam_' + mode, {'loss': loss.item(), 'unchanged': same})
        assert not same, same
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        ops.set_compute_dtype('bf16')


# ---------------------------------------------------------------------------------------------- 6. greedy decoding
GREEDY_BATCH = dict(batch=4, frames=200, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[200, 7, 97, 40], tgt_lengths=[10, 8, 10, 5])
GREEDY_SETTINGS = ((1, 200), (2, 200), (4, 200), (4, 3))        # (max_symbols, max_len)
_GREEDY = {}


def _greedy_weights():
    """seed and scales picked on the CPU so that every decision of every utterance is at least 1e-2 wide under all four settings: the
    output weight x 16, the predictor projection x 4 (the history then moves decisions) and + 10 on the blank's bias (frames end by
    arg-max as well as by the max_symbols limit)"""
    own = rr.transducer_weights(seed=24)
    own['joint.output.weight'] *= 16.0
    own['joint.pred_proj.weight'] *= 4.0
    own['joint.output.bias'][0] += 10.0
    return own


def _greedy_reference():
    """the float64 restatement of all four settings on the oracle's encoder output, computed once: {setting: [(tokens, frames, score, gap)]}"""
    if not _GREEDY:
        cfg = syn.c1_model(0.0)
        inputs, _ = syn.synthetic_batch(**GREEDY_BATCH)
        parts = H.filled_state(cfg, seed=21)
        with torch.no_grad():
            memory, mmask = _oracle_memory(inputs, parts, cfg)
        ref = rr.TransducerRef({k: v.double() for k, v in _greedy_weights().items()})
        pe, n = ref.project_encoder(memory.double()), mmask.sum(-1)
        _GREEDY['frames'] = n.tolist()
        for ms, ml in GREEDY_SETTINGS:
            _GREEDY[(ms, ml)] = [rr.rnnt_greedy_ref(pe[b], int(n[b]), ref.predict, ref.joint_logits, ms, ml) for b in range(pe.shape[0])]
    return _GREEDY


@pytest.mark.parametrize('max_symbols,max_len', GREEDY_SETTINGS)
def test_greedy_recognizer_equals_the_restatement(max_symbols, max_len):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    want = _greedy_reference()[(max_symbols, max_len)]
    frames = _greedy_reference()['frames']
    # before the device is touched: every decision of every utterance is wide, and the setting tests what it is there for
    assert min(w[3] for w in want) >= 1e-2, [w[3] for w in want]
    assert 1 in frames and max(frames) > 4 * min(frames)                          # a one-frame utterance; very different finishing steps
    if max_symbols == 1:                                                          # the forced frame advance shows: more tokens at 2
        assert any(len(a[0]) > len(b[0]) for a, b in zip(_greedy_reference()[(2, max_len)], want))
    if max_symbols == 4 and max_len == 200:                                       # and frames also end by arg-max after an emission
        assert any(len(w[0]) % 4 for w in want) and any(0 < len(w[0]) for w in want)
    if max_len == 3:
        assert all(len(w[0]) == 3 for w in want)                                  # truncation
    cfg = syn.c1_model(0.0)
    inputs, _ = syn.synthetic_batch(**GREEDY_BATCH)
    ops.set_compute_dtype('fp32')
    try:
        model = _load(ota.TransducerModel(rc.model_config()), H.filled_state(cfg, seed=21), _greedy_weights()).to(DEV)
        idx2unit = {i: 'u%d' % i for i in range(100)}
        rec = ota.TransducerRecognizer(model, idx2unit, max_symbols=max_symbols, max_len=max_len)
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        tokens, lengths, scores, fr = rec._decode(x, m)
        tok3, len3, sc3 = rec.recognize_tokens(x, m)
        texts, times = rec.recognize_with_times(x, m)
        torch.cuda.synchronize()
        tokens, lengths, scores, fr = tokens.cpu(), lengths.cpu(), scores.cpu(), fr.cpu()
        got = [(tokens[b, :int(lengths[b])].tolist(), fr[b, :int(lengths[b])].tolist(), float(scores[b])) for b in range(4)]
        s_err = [abs(g[2] - w[2]) / abs(w[2]) for g, w in zip(got, want)]
        _report('greedy', 'ms%d_len%d' % (max_symbols, max_len), {'lengths': lengths.tolist(), 'want_lengths': [len(w[0]) for w in want],
                                                                 'score_err': s_err, 'min_gap': min(w[3] for w in want)})
        assert tokens.shape == (4, max_len) and tokens.dtype == torch.int64 and lengths.dtype == torch.int32 and fr.dtype == torch.int32
        for b, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0] and g[1] == w[1], (b, g[0][:8], w[0][:8], g[1][:8], w[1][:8])
            assert s_err[b] <= 1e-4, (b, g[2], w[2])
            assert float(tokens[b, int(lengths[b]):].abs().max() if int(lengths[b]) < max_len else 0) == 0      # nothing behind a length
        assert tuple(tok3.shape) == (4, 1, max_len) and tuple(len3.shape) == (4, 1) and tuple(sc3.shape) == (4, 1)
        assert torch.equal(tok3[:, 0].cpu(), tokens) and torch.equal(len3[:, 0].cpu(), lengths)
        assert texts == rec.translate([g[0] for g in got]) == rec.recognize(x, m)
        for b in range(4):
            assert ' '.join(u for u, _ in times[b]) == texts[b]
            assert [t for _, t in times[b]] == [t for k, t in zip(got[b][0], got[b][1])][:len(times[b])]
    finally:
        ops.set_compute_dtype('bf16')


DEEP_BATCH = dict(batch=4, frames=40, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[40, 7, 23, 15], tgt_lengths=[10, 8, 10, 5])
DEEP_LAYERS = 8


def _deep_weights():
    """an 8-layer predictor (17 commit items in fp32, 25 in the 16-bit modes: more than one commit call); seed and scales picked on
    the CPU so that every decision is at least 0.15 wide, an order above what fp16 operands move a logit by"""
    own = rr.transducer_weights(seed=41, layers=DEEP_LAYERS)
    own['joint.output.weight'] *= 16.0
    own['joint.pred_proj.weight'] *= 4.0
    own['joint.output.bias'][0] += 6.0
    return own


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])          # bf16 operands move a logit by about half of the 0.15 gap: no exact claim there
def test_greedy_decoding_in_fp16_and_with_a_deep_predictor(mode):
    """the 16-bit path of the loop -- z16 from the step's joint, the twins of h in the commit table, the twin the output GEMM reads --
    and a commit table longer than one call takes: tokens and frames equal to the float64 restatement in every mode"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    if 'deep' not in _GREEDY:
        cfg = syn.c1_model(0.0)
        inputs, _ = syn.synthetic_batch(**DEEP_BATCH)
        with torch.no_grad():
            memory, mmask = _oracle_memory(inputs, H.filled_state(cfg, seed=21), cfg)
        ref = rr.TransducerRef({k: v.double() for k, v in _deep_weights().items()}, layers=DEEP_LAYERS)
        pe, n = ref.project_encoder(memory.double()), mmask.sum(-1)
        _GREEDY['deep'] = [rr.rnnt_greedy_ref(pe[b], int(n[b]), ref.predict, ref.joint_logits, 2, 50) for b in range(4)]
    want = _GREEDY['deep']
    assert min(w[3] for w in want) >= 0.15 and sum(len(w[0]) for w in want) >= 30, [(len(w[0]), w[3]) for w in want]
    cfg = syn.c1_model(0.0)
    inputs, _ = syn.synthetic_batch(**DEEP_BATCH)
    mc = rc.model_config()
    mc['predictor']['num_layers'] = DEEP_LAYERS
    ops.set_compute_dtype(mode)
    try:
        model = _load(ota.TransducerModel(mc), H.filled_state(cfg, seed=21), _deep_weights()).to(DEV)
        rec = ota.TransducerRecognizer(model, {i: 'u%d' % i for i in range(100)}, max_symbols=2, max_len=50)
        tokens, lengths, scores, fr = (t.cpu() for t in rec._decode(inputs['inputs'].to(DEV), inputs['mask'].to(DEV)))
        got = [(tokens[b, :int(lengths[b])].tolist(), fr[b, :int(lengths[b])].tolist(), float(scores[b])) for b in range(4)]
        s_err = [abs(g[2] - w[2]) / abs(w[2]) for g, w in zip(got, want)]
        _report('greedy', 'deep_' + mode, {'lengths': lengths.tolist(), 'want_lengths': [len(w[0]) for w in want], 'score_err': s_err,
                                           'min_gap': min(w[3] for w in want)})
        for b, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0] and g[1] == w[1], (mode, b, g[0][:8], w[0][:8], g[1][:8], w[1][:8])
            assert s_err[b] <= (1e-4 if mode == 'fp32' else 2e-2), (mode, b, g[2], w[2])
    finally:
        ops.set_compute_dtype('bf16')


def test_evaluate_runs_on_the_transducer_recognizer():
    """evaluate.evaluate works on the recognizer as it stands: recognize_tokens feeds the device edit distance"""
    import opentransformer_amd as ota
    from opentransformer_amd import evaluate, ops
    cfg = syn.c1_model(0.0)
    inputs, targets = syn.synthetic_batch(**GREEDY_BATCH)
    ops.set_compute_dtype('fp16')
    try:
        model = _load(ota.TransducerModel(rc.model_config()), H.filled_state(cfg, seed=21), _greedy_weights()).to(DEV)
        rec = ota.TransducerRecognizer(model, {i: 'u%d' % i for i in range(100)}, max_symbols=1, max_len=20)
        out = evaluate.evaluate(rec, [(['a', 'b', 'c', 'd'], to_dev(inputs), to_dev(targets))])
        torch.cuda.synchronize()
        assert isinstance(out, dict) and out
    finally:
        ops.set_compute_dtype('bf16')
