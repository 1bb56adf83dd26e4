"""GPU (-m gpu): the CTC loss kernel (csrc/ctc.hip) and otr_log_softmax against float64 on the CPU, per utterance.

The kernel runs one thread per extended-label state; everything up to this file kept its live states inside the first wavefront.
The cases (tests/ctc_loss_cases.py, checked on the CPU by tests/test_ctc_loss_cases.py) put live states, the last of them and a
repeated label pair on both sides of every wave boundary up to the advertised 127 labels, and walk the degenerate ends.

Judged per utterance, never by one norm over the batch: the loss is mean_b(nll_b / L_b), so the slab of a long target is scaled
by 1 / (B L_b) and drowns in a batch norm.  Bound: err_b <= K * floor_b + tiny_b, floor_b the distance of float32 F.ctc_loss on the
CPU from float64 on the same inputs, tiny_b = T_b * eps_fp32 * max |lp_b| (ctc_loss_cases.tiny).  Every test writes the figures it
measured into parity_out/ctc_loss_parity.json (or under $OTR_PARITY_DIR) before it asserts."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import ctc_loss_cases as cc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# err_b <= K * floor_b + tiny_b.  A different summation order inside lse3 and the atomics may cost a small factor over the reference's
# own float32 rounding, not an order of magnitude.  Measured on MI355X (profiles/ctc_loss_parity.json), worst over all cases and
# utterances: gradient slab 1.70 x its floor (blank_last, L 33), 2 x that rounded up = 4.  Frame column sums reach 3.6 x the gradient's
# floor where the recursion runs and 6.1 x in the one-frame utterances of empty_and_short, where both sides are a few eps_fp32 (tiny
# carries those).  nll is ONE float32 number per utterance: its ratio exceeds 4 (worst 29, blank_mid) only where the CPU's float32
# value happens to land within a tenth of a float32 ulp of float64 (floors of 5e-9 .. 3e-8 relative against an ulp of 6e-8 .. 1.2e-7),
# so the ratio measures the reference's luck; tiny_b over nll_b (about 4 ulp) is what bounds the kernel there.
K = 4.0
REPORT = {}


def _report(name, tag, rec):
    REPORT.setdefault(name, {})[tag] = rec
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'ctc_loss_parity.json'), 'w') as f:
        json.dump(json.loads(json.dumps(REPORT), parse_float=lambda x: float('%.3g' % float(x))), f, sort_keys=True, indent=None,
                  separators=(',', ':'))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_fn(c, in_len=None, tgt_len=None):
    """ops.CTCLossFn as the model calls it: (loss, d loss / d logits) on the device"""
    from opentransformer_amd import ops
    x = c['logits'].to(DEV).requires_grad_(True)
    il = (c['in_len'] if in_len is None else in_len).to(DEV)
    tl = (c['tgt_len'] if tgt_len is None else tgt_len).to(DEV)
    loss = ops.CTCLossFn.apply(x, c['targets'].to(DEV), il, tl, c['blank'])
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def run_direct(c, in_len=None, tgt_len=None, grad=True, wide=0, nan_ws=False):
    """otr_ctc_loss itself on ops.log_softmax(logits): (loss, nll[B], dlogits or None) on the device.  wide > 0: the targets are the
    [:, 1:-1]-like view of a matrix `wide` columns wider whose other columns hold a valid label that is not in the view (a wrong row
    stride reads those and changes the result; it cannot fault).  nan_ws: the alpha workspace starts as NaN."""
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    B, T, V = c['logits'].shape
    lp = ops.log_softmax(c['logits'].to(DEV))
    W = c['targets'].shape[1]
    if wide:
        poison = (c['blank'] + 1 + int(c['targets'][0, 0])) % V
        poison = poison if poison != c['blank'] else (poison + 1) % V
        big = torch.full((B, W + wide), poison, dtype=torch.int64)
        big[:, 1:1 + W] = c['targets']
        big = big.to(DEV)
        tg = big[:, 1:1 + W]
        assert tg.stride(0) == W + wide and tg.stride(1) == 1
    else:
        tg = c['targets'].to(DEV).contiguous()
    il = (c['in_len'] if in_len is None else in_len).to(torch.int32).to(DEV)
    tl = (c['tgt_len'] if tgt_len is None else tgt_len).to(torch.int32).to(DEV)
    ws = torch.full((B, T, 2 * W + 1), float('nan') if nan_ws else 0.0, dtype=torch.float32, device=DEV)
    nll = torch.full((B,), -7.0, dtype=torch.float32, device=DEV)
    loss = torch.full((), -7.0, dtype=torch.float32, device=DEV)
    dl = torch.full((B, T, V), -7.0, dtype=torch.float32, device=DEV) if grad else None
    ret = L.load().otr_ctc_loss(_p(lp), _p(tg), tg.stride(0), _p(il), _p(tl), B, T, V, W, c['blank'], _p(ws), _p(nll), _p(loss), _p(dl),
                                _stream())
    L.check(ret, 'otr_ctc_loss')
    torch.cuda.synchronize()
    return loss, nll, dl


def check_against_reference(name, tag, loss, nll, g):
    """loss, nll per utterance (None through the autograd function, which does not return it) and the gradient per utterance slab
    against float64; the exact structure; the column sum of every live frame.  Figures are written out before anything is asserted."""
    c = cc.build(name)
    B, T, V = c['logits'].shape
    ref_loss, ref_nll, ref_g = cc.reference_of(name)
    fl, tn = cc.floor_of(name), cc.tiny_of(name)
    feas = cc.feasible(c)
    il, tl, _ = cc.effective_lengths(c['targets'], c['in_len'], c['tgt_len'], T)
    cf = cc.coef(c['tgt_len'], c['targets'], B)
    g = g.detach().cpu()
    e_grad = cc.slab_rel(g, ref_g)
    e_rows = cc.rowsum_rel(g, il, cf)
    e_nll = cc.nll_rel(nll, ref_nll) if nll is not None else None
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    tiny_nll = tn / ref_nll.abs().clamp_min(1e-300)
    tiny_loss = float((tn / tl.clamp_min(1)).mean() / ref_loss.abs())

    def ratios(e, f):
        return [float(e[b] / f[b]) if float(f[b]) > 0 else None for b in range(B)]

    rec = {'shape': [B, T, V], 'tgt_len': c['tgt_len'].tolist(), 'K': K, 'loss_err': e_loss, 'loss_floor': fl['loss'], 'loss_tiny': tiny_loss,
           'grad_err': e_grad.tolist(), 'grad_floor': fl['grad'].tolist(), 'tiny': tn.tolist(), 'grad_err_over_floor': ratios(e_grad, fl['grad']),
           'rowsum_err': e_rows.tolist(), 'rowsum_of_the_float32_reference': fl['rowsum'].tolist(), 'rowsum_err_over_floor': ratios(e_rows, fl['grad'])}
    if e_nll is not None:
        rec.update(nll_err=e_nll.tolist(), nll_floor=fl['nll'].tolist(), nll_tiny=tiny_nll.tolist(), nll_err_over_floor=ratios(e_nll, fl['nll']))
    for k in ('grad', 'rowsum', 'nll'):
        r = [x for x in rec.get(k + '_err_over_floor', []) if x is not None]
        rec['max_%s_err_over_floor' % k] = max(r) if r else None
    _report(name, tag, rec)
    print(name, tag, json.dumps({k: v for k, v in rec.items() if k.startswith('max_') or k.startswith('loss_')}))

    assert bool(torch.isfinite(g).all()), (name, tag)
    for b in range(B):                                                           # utterances first: a failure names one, and a frame
        where = (name, tag, 'utterance %d' % b, 'L %d' % int(c['tgt_len'][b]), 'T_b %d' % int(il[b]))
        if int(il[b]) < T:                                                       # frames past in_len: exactly zero
            assert float(g[b, int(il[b]):].abs().max()) == 0.0, where + ('frames past in_len',)
        if not feas[b]:                                                          # infeasible / guarded: nll 0, the whole slab zero
            assert float(g[b].abs().max()) == 0.0, where + ('slab of an utterance without alignment',)
            assert nll is None or float(nll[b]) == 0.0, where + ('nll', float(nll[b]))
            continue
        if nll is not None:
            assert float(e_nll[b]) <= K * float(fl['nll'][b]) + float(tiny_nll[b]), \
                where + ('nll', float(nll[b]), float(ref_nll[b]), float(e_nll[b]), float(fl['nll'][b]), float(tiny_nll[b]))
        if not float(e_grad[b]) <= K * float(fl['grad'][b]) + float(tn[b]):
            per_t = (g[b].double() - ref_g[b]).norm(dim=1)
            t = int(per_t.argmax())
            v = int((g[b, t].double() - ref_g[b, t]).abs().argmax())
            raise AssertionError(where + ('gradient slab', float(e_grad[b]), 'floor', float(fl['grad'][b]), 'tiny', float(tn[b]),
                                          'worst frame %d column %d: got %.6e want %.6e' % (t, v, float(g[b, t, v]), float(ref_g[b, t, v]))))
        # 1 - sum_s gamma_t(s), the relative error of a frame's occupancies: bounded like the gradient, by the gradient's floor.  The
        # float32 reference's own column sums say nothing here: autograd's log_softmax backward subtracts softmax * sum_v(d lp) and so
        # projects them to 1e-7 whatever the recursion did (recorded as rowsum_of_the_float32_reference), while the fused form
        # coef * (softmax - occupancy) keeps the residual; both are the exact gradient plus an error of the size of that residual.
        assert float(e_rows[b]) <= K * float(fl['grad'][b]) + float(tn[b]), \
            where + ('sum_v dlogits / coef', float(e_rows[b]), float(fl['grad'][b]), float(tn[b]))
    assert e_loss <= K * fl['loss'] + tiny_loss, (name, tag, 'loss', float(loss), float(ref_loss), e_loss, fl['loss'], tiny_loss)


def single_state_columns(c, b):
    """columns of utterance b that exactly one state maps to (labels that occur once in its target): one atomicAdd per frame"""
    L = int(c['tgt_len'][b])
    if not 0 < L <= c['targets'].shape[1]:
        return torch.zeros(0, dtype=torch.int64)
    u, n = torch.unique(c['targets'][b, :L], return_counts=True)
    return u[n == 1]


def check_same_result(name, tag, a, b, utterances=None):
    """two launches that must compute the same thing: nll bit-equal (no atomics), slabs within 2 * tiny of each other and bit-equal
    in every single-state column; the blank column collects up to L + 1 atomicAdds per frame in a free order"""
    c = cc.build(name)
    tn = cc.tiny_of(name)
    (_, nll_a, g_a), (_, nll_b, g_b) = a, b
    for u in (range(c['logits'].shape[0]) if utterances is None else utterances):
        assert torch.equal(nll_a[u], nll_b[u]), (name, tag, 'utterance %d' % u, 'nll', float(nll_a[u]), float(nll_b[u]))
        if g_a is None or g_b is None:
            continue
        d = float((g_a[u].double() - g_b[u].double()).norm())
        n = float(g_a[u].double().norm())
        assert d <= 2 * float(tn[u]) * n, (name, tag, 'utterance %d' % u, 'slabs', d / max(n, 1e-300))
        cols = single_state_columns(c, u).to(DEV)
        assert torch.equal(g_a[u][:, cols], g_b[u][:, cols]), (name, tag, 'utterance %d' % u, 'single-state columns')


def check_loss_close(name, tag, la, lb):
    """the scalar is an atomic sum over utterances: equal up to the order of B float32 additions"""
    B = cc.build(name)['logits'].shape[0]
    assert abs(float(la) - float(lb)) <= B * cc.EPS32 * abs(float(la)), (name, tag, float(la), float(lb))


# ------------------------------------------------------------------------------------------ every case, both ways in
@pytest.mark.parametrize('name', cc.NAMES)
def test_ctc_loss_fn_matches_float64(name):
    c = cc.build(name)
    loss, g = run_fn(c)
    check_against_reference(name, 'CTCLossFn', loss, None, g)
    # the loss-only path (logits without a gradient: dlogits == NULL)
    from opentransformer_amd import ops
    only = ops.CTCLossFn.apply(c['logits'].to(DEV), c['targets'].to(DEV), c['in_len'].to(DEV), c['tgt_len'].to(DEV), c['blank'])
    check_loss_close(name, 'CTCLossFn loss only', loss, only)


@pytest.mark.parametrize('name', cc.NAMES)
def test_ctc_entry_direct_matches_float64(name):
    c = cc.build(name)
    first = run_direct(c)
    check_against_reference(name, 'otr_ctc_loss', *first)
    again = run_direct(c)
    check_same_result(name, 'second launch', first, again)
    check_loss_close(name, 'second launch', first[0], again[0])
    view = run_direct(c, wide=3, nan_ws=True)                       # ldt = max_tgt + 3, workspace NaN
    check_same_result(name, 'ldt > max_tgt, NaN workspace', first, view)
    check_loss_close(name, 'ldt > max_tgt, NaN workspace', first[0], view[0])
    only = run_direct(c, grad=False, nan_ws=True)                   # dlogits == NULL
    check_same_result(name, 'loss only', first, only)
    check_loss_close(name, 'loss only', first[0], only[0])
    loss_fn, g_fn = run_fn(c)                                       # and the autograd function is this entry
    check_same_result(name, 'CTCLossFn against the entry', first, (None, first[1], g_fn))
    check_loss_close(name, 'CTCLossFn against the entry', first[0], loss_fn)


# ------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize('name', ['one_frame_short', 'empty_and_short', 'tgt_len_guard'])
def test_neighbours_of_an_utterance_without_alignment_are_untouched(name):
    """the same batch with the infeasible / guarded utterances given enough frames / a target length inside the padded width: every
    other utterance keeps its nll bit for bit and its slab to the two-launch tolerance"""
    c = cc.build(name)
    B = c['logits'].shape[0]
    feas = cc.feasible(c)
    got = run_direct(c)
    raised_case = dict(c, in_len=c['raised_in_len'] if c['raised_in_len'] is not None else c['in_len'],
                       tgt_len=c.get('raised_tgt_len', c['tgt_len']))
    raised = run_direct(c, in_len=raised_case['in_len'], tgt_len=raised_case['tgt_len'])
    changed = [b for b in range(B) if int(raised_case['in_len'][b]) != int(c['in_len'][b]) or int(raised_case['tgt_len'][b]) != int(c['tgt_len'][b])]
    assert set(changed) == set(c['infeasible']) | set(c['guarded']) and changed
    for b in changed:
        assert not feas[b] and float(got[1][b]) == 0.0 and float(got[2][b].abs().max()) == 0.0, (name, b)
        assert float(raised[1][b]) > 0.0 and float(raised[2][b].abs().max()) > 0.0, (name, b)       # and it is the length that did it
    check_same_result(name, 'neighbours', got, raised, utterances=[b for b in range(B) if b not in changed])
    # the scalar holds the feasible utterances only
    cf = cc.coef(c['tgt_len'], c['targets'], B)
    want = float((got[1].double().cpu() * cf).sum())
    assert abs(float(got[0]) - want) <= (B + 4) * cc.EPS32 * abs(want), (name, float(got[0]), want)      # coef, the product, B additions


def test_in_len_beyond_T_is_clamped():
    c = cc.build('in_len_clamp')
    got = run_direct(c)
    clamped = run_direct(c, in_len=c['clamped_in_len'])
    check_same_result('in_len_clamp', 'in_len > T against in_len = T', got, clamped)
    check_loss_close('in_len_clamp', 'in_len > T against in_len = T', got[0], clamped[0])


def test_single_path_is_the_closed_form():
    """one alignment: the occupancies are 1 on it, so the slab is coef * (softmax - onehot(path)) with no recursion noise left"""
    c = cc.build('single_path')
    tn = cc.tiny_of('single_path')
    _, nll, g = run_direct(c)
    for b in c['single_path']:
        want_nll, want_g = cc.single_path_closed_form(c, b)
        assert abs(float(nll[b]) - float(want_nll)) <= float(tn[b]), (b, float(nll[b]), float(want_nll))
        e = float((g[b].double().cpu() - want_g).norm() / want_g.norm())
        assert e <= float(tn[b]), (b, e, float(tn[b]))


# ------------------------------------------------------------------------------------------ contract
def test_target_width_limit():
    """a padded target width of 128 (S = 257 states) is refused before anything is launched; 127 runs (the waves_* cases)"""
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    B, T, V = 2, 300, 20
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, V, generator=g).to(DEV)
    tg = torch.randint(1, V, (B, 128), generator=g).to(DEV)
    il = torch.tensor([T, T], device=DEV)
    with pytest.raises(L.OtransHipError, match='127'):
        ops.CTCLossFn.apply(x.clone().requires_grad_(True), tg, il, torch.tensor([128, 5], device=DEV), 0)
    with pytest.raises(L.OtransHipError, match='127'):
        ops.CTCLossFn.apply(x.clone().requires_grad_(True), tg, il, torch.tensor([5, 5], device=DEV), 0)      # the width decides, not the lengths
    lp = ops.log_softmax(x)
    il32, tl32 = il.to(torch.int32), torch.tensor([5, 5], dtype=torch.int32, device=DEV)
    ws = torch.full((B, T, 257), 3.0, device=DEV)
    nll, loss, dl = torch.full((B,), 3.0, device=DEV), torch.full((), 3.0, device=DEV), torch.full((B, T, V), 3.0, device=DEV)
    ret = L.load().otr_ctc_loss(_p(lp), _p(tg), 128, _p(il32), _p(tl32), B, T, V, 128, 0, _p(ws), _p(nll), _p(loss), _p(dl), _stream())
    assert ret != 0
    msg = L.load().otr_last_error_string().decode()
    assert 'ctc_loss' in msg and '128' in msg and '127' in msg, msg
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in (ws, nll, loss, dl))                                    # nothing ran
    ret = L.load().otr_ctc_loss(_p(lp), _p(tg), 128, _p(il32), _p(tl32), B, T, V, 127, 0, _p(ws), _p(nll), _p(loss), _p(dl), _stream())
    assert ret == 0
    torch.cuda.synchronize()
    assert bool((nll > 0).all()) and float(loss) > 0 and bool(torch.isfinite(dl).all())


def test_compute_mode_does_not_enter():
    """the loss is fp32 throughout: under bf16 and fp16 (the second build of the library) it is the fp32-mode result"""
    from opentransformer_amd import ops
    name = 'waves_v50'
    c = cc.build(name)
    try:
        ops.set_compute_dtype('fp32')
        base = run_direct(c)
        for mode in ('bf16', 'fp16'):
            ops.set_compute_dtype(mode)
            got = run_direct(c)
            check_same_result(name, mode, base, got)
            check_loss_close(name, mode, base[0], got[0])
            loss, g = run_fn(c)
            check_same_result(name, mode + ' CTCLossFn', base, (None, base[1], g))
            check_loss_close(name, mode + ' CTCLossFn', base[0], loss)
    finally:
        ops.set_compute_dtype('bf16')


# ------------------------------------------------------------------------------------------ log_softmax
def _log_softmax_rows(V, seed):
    """rows that go wrong in a log-softmax: plain, one dominant logit, shifted by +-1e4, -inf entries"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(7, V, generator=g) * 3.0
    x[1] = -80.0
    x[1, V // 2] = 80.0                              # lse = 80 exactly: the rest of the row is -160
    x[2] += 1e4
    x[3] -= 1e4
    if V > 1:
        x[4, ::2] = float('-inf')                    # finite elsewhere (the odd columns)
        x[5, :V - 1] = float('-inf')                 # a single finite entry: y = 0 there
    return x


def _check_log_softmax(x, y, what):
    """|y - ref| per row, absolute, against K times the float32 torch.log_softmax error on the same row plus the rounding of the
    result itself (eps_fp32 * max |ref| over the row: y is a float32)"""
    ref = torch.log_softmax(x.double().cpu(), -1)
    f32 = torch.log_softmax(x.float().cpu(), -1).double()
    y = y.cpu().double()
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(y) & (y < 0), inf) and not bool(torch.isnan(y).any()), what
    z = torch.zeros_like(ref)
    err = torch.where(inf, z, (y - ref).abs()).max(dim=-1).values
    flo = torch.where(inf, z, (f32 - ref).abs()).max(dim=-1).values
    tny = cc.EPS32 * torch.where(inf, z, ref.abs()).max(dim=-1).values
    for r in range(ref.shape[0]):
        assert float(err[r]) <= K * float(flo[r]) + float(tny[r]), (what, 'row %d' % r, float(err[r]), float(flo[r]), float(tny[r]))


@pytest.mark.parametrize('V', [1, 2, 63, 64, 65, 255, 256, 257, 4233, 4234, 8191])
def test_log_softmax_matches_float64(V):
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    x = _log_softmax_rows(V, 100 + V).to(DEV)
    _check_log_softmax(x, ops.log_softmax(x), ('ops.log_softmax', V))
    y = torch.full_like(x, 5.0)
    L.check(L.load().otr_log_softmax(_p(x), _p(y), x.shape[0], V, _stream()), 'otr_log_softmax')
    _check_log_softmax(x, y, ('otr_log_softmax', V))
    wide = torch.full((7, 2 * V + 3), 9.0, device=DEV)              # a non-contiguous view: every other column of a wider matrix
    wide[:, 1:1 + 2 * V:2] = x
    view = wide[:, 1:1 + 2 * V:2]
    assert not view.is_contiguous() or V == 1
    _check_log_softmax(x, ops.log_softmax(view), ('view', V))
    x3 = x.reshape(7, 1, V).expand(7, 2, V)                          # [.., V] of any rank
    assert torch.equal(ops.log_softmax(x3)[:, 1], ops.log_softmax(x))


def test_log_softmax_of_no_rows():
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    y = ops.log_softmax(torch.zeros(0, 37, device=DEV))
    assert tuple(y.shape) == (0, 37)
    keep = torch.full((4,), 2.0, device=DEV)
    L.check(L.load().otr_log_softmax(_p(keep), _p(keep), 0, 4, _stream()), 'otr_log_softmax')
    torch.cuda.synchronize()
    assert bool((keep == 2.0).all())
