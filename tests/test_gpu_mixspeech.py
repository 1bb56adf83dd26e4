"""GPU (-m gpu): MixSpeech.  otr_mixspeech_mix bit for bit against the float32 numpy composition (tests/mixspeech_ref.py); otr_ctc_loss_pair
per utterance against float64 on the CPU, with the bound of tests/test_gpu_ctc_loss.py (err <= K * floor + tiny, K = 4, floor the float32
CPU composition's distance from float64, tiny = ctc_loss_cases.tiny), its feasibility rules and its limits lam = 1 and lam = 0 against
otr_ctc_loss; MixSpeechTraining against the CPU oracle composite lam * oracle(mixed, t1) + (1 - lam) * oracle(mixed, t2), in eval(), on
identical pairs and under hipGraph replay.  The CTC tests write the worst ratios they measured to parity_out/mixspeech_parity.json (or
under $OTR_PARITY_DIR) before they assert."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import ctc_loss_cases as cc
from tests import helpers as H
from tests import mixspeech_ref as ref
from tests.test_gpu_ctc_loss import K, check_same_result, run_direct
from tests.test_gpu_model import TOL16

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lam_dev(lam):
    return torch.tensor([float(np.float32(lam))], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------ the mix kernel
def _shifted(shape, dtype, shift, fill):
    """a tensor of `shape` whose base lies `shift` elements of 4 bytes behind a 16-byte boundary"""
    n = int(np.prod(shape))
    flat = torch.full((n + 4,), fill, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    return flat[shift:shift + n].view(shape)


def _run_mix(x, lengths, lam, shift=0):
    """otr_mixspeech_mix itself, every output pre-filled with a value it never writes"""
    from opentransformer_amd import _lib as L
    B, T, F = x.shape
    P = B // 2
    xd = _shifted((B, T, F), torch.float32, shift, 0.0)
    xd.copy_(torch.from_numpy(x))
    out = _shifted((P, T, F), torch.float32, shift, -7.0)
    out_len = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    mask = torch.full((P, T), 7, dtype=torch.uint8, device=DEV)
    if shift:
        assert xd.data_ptr() % 16 == 4 * shift and out.data_ptr() % 16 == 4 * shift
    n, lam_d = torch.from_numpy(np.asarray(lengths, np.int32)).to(DEV), _lam_dev(lam)
    L.check(L.load().otr_mixspeech_mix(_p(xd), T * F, _p(n), _p(lam_d), B, T, F, _p(out), _p(out_len), _p(mask), _stream()),
            'otr_mixspeech_mix')
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy(), mask.cpu().numpy()


def _length_patterns(B, T, rng):
    """per pair (first, second): equal, first longer, second longer, one of them T, one of them 0 -- every pattern on pair 0 in turn,
    the other pairs (and an odd last utterance) drawn"""
    short, mid = max(T // 3, 0), max(2 * T // 3, min(T, 1))
    for first, second in ((mid, mid), (mid, short), (short, mid), (T, short), (short, T), (0, mid), (mid, 0), (0, 0)):
        n = rng.integers(0, T + 1, B)
        n[0], n[1] = first, second
        yield n


def _lams(seed):
    np.random.seed(seed)
    return [0.0, 1.0, 0.5, 0.3, float(np.float32(np.random.beta(0.5, 0.5, size=(1))[0]))]


def _check_mix(x, n, lam, shift=0):
    want, want_len, want_mask = ref.mix_pairs(x, n, lam)
    poisoned = np.where(np.arange(x.shape[1])[None, :, None] < np.clip(n, 0, x.shape[1])[:, None, None], x, np.float32('nan'))
    got, got_len, got_mask = _run_mix(poisoned, n, lam, shift)
    where = (x.shape, n.tolist(), lam, shift)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), where       # bit for bit; a NaN read from the padding would show
    assert np.array_equal(got_len, want_len) and np.array_equal(got_mask, want_mask.astype(np.uint8)), where
    for p in range(x.shape[0] // 2):
        assert not got[p, int(want_len[p]):].any(), where                        # frames past the pair's length: exactly zero


@pytest.mark.parametrize('F', [1, 3, 80, 83])
@pytest.mark.parametrize('T', [1, 7, 96])
@pytest.mark.parametrize('B', [2, 3, 5, 8])
def test_mix_kernel_is_the_float32_composition_bit_for_bit(B, T, F):
    rng = np.random.default_rng(B * 10000 + T * 100 + F)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    lams = _lams(B + T + F)
    assert 0.0 < lams[-1] < 1.0
    for n in _length_patterns(B, T, rng):
        for lam in lams:
            _check_mix(x, n, lam)


@pytest.mark.parametrize('B,T,F', [(5, 96, 80), (4, 7, 83), (2, 1, 1)])
def test_mix_kernel_with_bases_off_a_16_byte_boundary(B, T, F):
    rng = np.random.default_rng(B + T + F)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    for n in _length_patterns(B, T, rng):
        _check_mix(x, n, 0.3, shift=1)


def test_ops_mixspeech_mix_reads_views_and_clamps_lengths():
    from opentransformer_amd import ops
    rng = np.random.default_rng(3)
    B, T, F = 5, 9, 6
    big = torch.from_numpy(rng.standard_normal((B, T + 2, F)).astype(np.float32)).to(DEV)
    view = big[:, :T]                                                    # utterance pitch (T + 2) * F, no copy
    n = np.array([T + 5, -3, 4, 9, 2])
    out, out_len, mask = ops.mixspeech_mix(view, torch.from_numpy(n).to(DEV), _lam_dev(0.3))
    want, want_len, want_mask = ref.mix_pairs(view.cpu().numpy(), n, 0.3)
    assert mask.dtype == torch.bool and out_len.dtype == torch.int32 and not out.requires_grad
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(out_len.cpu().numpy(), want_len)
    assert np.array_equal(mask.cpu().numpy(), want_mask)


# ------------------------------------------------------------------------------------------ the paired CTC loss
def _report(name, tag, rec):
    REPORT.setdefault(name, {})[tag] = rec
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mixspeech_parity.json'), 'w') as f:
        json.dump(json.loads(json.dumps(REPORT), parse_float=lambda x: float('%.3g' % float(x))), f, sort_keys=True, indent=None,
                  separators=(',', ':'))


def run_pair(name, lam, in_len=None, tgt_len_a=None, tgt_len_b=None, grad=True):
    """otr_ctc_loss_pair itself on ops.log_softmax(logits): (loss3, nll [2, P], dlogits or None) on the device.  The two label sets are
    the even and the odd rows of ONE [2P, W] matrix, passed as they lie (row stride 2W); workspace and outputs start as NaN / -7."""
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    a, b = ref.pair_of(name)
    P, T, V = a['logits'].shape
    W = a['targets'].shape[1]
    lp = ops.log_softmax(a['logits'].to(DEV))
    both = torch.stack((a['targets'], b['targets']), dim=1).reshape(2 * P, W).to(DEV)
    ta, tb = both[0::2], both[1::2]
    assert ta.stride(0) == 2 * W and tb.data_ptr() == ta.data_ptr() + 8 * W
    i32 = lambda t: t.to(torch.int32).to(DEV)                            # noqa: E731
    il = i32(a['in_len'] if in_len is None else in_len)
    la = i32(a['tgt_len'] if tgt_len_a is None else tgt_len_a)
    lb = i32(b['tgt_len'] if tgt_len_b is None else tgt_len_b)
    ws = torch.full((2, P, T, 2 * W + 1), float('nan'), dtype=torch.float32, device=DEV)
    nll = torch.full((2, P), -7.0, dtype=torch.float32, device=DEV)
    loss3 = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    dl = torch.full((P, T, V), -7.0, dtype=torch.float32, device=DEV) if grad else None
    lam_d = _lam_dev(lam)
    L.check(L.load().otr_ctc_loss_pair(_p(lp), _p(ta), 2 * W, _p(la), _p(tb), 2 * W, _p(lb), _p(il), _p(lam_d), P, T, V, W, a['blank'],
                                       _p(ws), _p(nll), _p(loss3), _p(dl), _stream()), 'otr_ctc_loss_pair')
    torch.cuda.synchronize()
    return loss3, nll, dl


def check_pair_against_reference(name, lam, loss3, nll, g):
    """per utterance: nll per set, the gradient slab and the frame column sums; then the three losses.  err <= K * floor + tiny."""
    a, b = ref.pair_of(name)
    P, T, V = a['logits'].shape
    r, fl, tn = ref.reference_of(name, lam), ref.floor_of(name, lam), cc.tiny_of(name)
    feas = (cc.feasible(a), cc.feasible(b))
    il, _, _ = cc.effective_lengths(a['targets'], a['in_len'], a['tgt_len'], T)
    il = a['in_len'].long().clamp(0, T)                                  # frames, whatever a set's target length is
    cf = ref.pair_coef(a, b, lam)
    g = g.detach().cpu()
    nll = nll.detach().cpu()
    e_grad = cc.slab_rel(g, r['grad'])
    e_rows = cc.rowsum_rel(g, il, cf.clamp_min(1e-300))
    e_nll = torch.stack([cc.nll_rel(nll[k], r['nll'][k]) for k in (0, 1)])
    tiny_nll = tn[None, :] / r['nll'].abs().clamp_min(1e-300)
    w = (float(np.float32(lam)), float(np.float32(1) - np.float32(lam)))
    tl = [cc.effective_lengths(c['targets'], c['in_len'], c['tgt_len'], T)[1].clamp_min(1).double() for c in (a, b)]
    tiny_k = [float((tn / tl[k]).mean()) for k in (0, 1)]
    got_loss = {'loss': float(loss3[0]), 'loss_a': float(loss3[1]), 'loss_b': float(loss3[2])}
    tiny_loss = {'loss': w[0] * tiny_k[0] + w[1] * tiny_k[1], 'loss_a': tiny_k[0], 'loss_b': tiny_k[1]}
    e_loss = {k: abs(v - float(r[k])) / max(abs(float(r[k])), 1e-300) for k, v in got_loss.items()}

    def worst(e, f):
        q = [float(e[i] / f[i]) for i in range(len(e)) if float(f[i]) > 0]
        return max(q) if q else None
    rec = {'shape': [P, T, V], 'lam': lam, 'K': K, 'max_grad_err_over_floor': worst(e_grad, fl['grad']),
           'max_rowsum_err_over_floor': worst(e_rows, fl['grad']),
           'max_nll_err_over_floor': worst(e_nll.flatten(), fl['nll'].flatten()),
           'loss_err': e_loss, 'loss_floor': {k: fl[k] for k in e_loss},
           'loss_tiny': {k: tiny_loss[k] / max(abs(float(r[k])), 1e-300) for k in e_loss}}
    _report(name, 'lam %g' % lam, rec)
    print(name, lam, json.dumps(rec))

    assert bool(torch.isfinite(g).all()), (name, lam)
    for p in range(P):
        where = (name, lam, 'utterance %d' % p, 'feasible (a, b) %s' % ((feas[0][p], feas[1][p]),))
        if int(il[p]) < T:
            assert float(g[p, int(il[p]):].abs().max()) == 0.0, where + ('frames past in_len',)
        for k in (0, 1):
            if not feas[k][p]:
                assert float(nll[k, p]) == 0.0, where + ('nll of set %d' % k, float(nll[k, p]))
            else:
                assert float(e_nll[k, p]) <= K * float(fl['nll'][k, p]) + float(tiny_nll[k, p]), \
                    where + ('nll of set %d' % k, float(nll[k, p]), float(r['nll'][k, p]), float(e_nll[k, p]), float(fl['nll'][k, p]))
        if not (feas[0][p] or feas[1][p]) or float(cf[p]) == 0.0:
            assert float(g[p].abs().max()) == 0.0, where + ('slab without any alignment, or with weight zero on the only one',)
            continue
        # the slab is the other set's gradient alone where one set has no alignment: that is what the reference's slab is there
        assert float(e_grad[p]) <= K * float(fl['grad'][p]) + float(tn[p]), \
            where + ('gradient slab', float(e_grad[p]), 'floor', float(fl['grad'][p]), 'tiny', float(tn[p]))
        assert float(e_rows[p]) <= K * float(fl['grad'][p]) + float(tn[p]), \
            where + ('sum_v dlogits / coef', float(e_rows[p]), float(fl['grad'][p]), float(tn[p]))
    for k in e_loss:
        assert e_loss[k] <= K * fl[k] + tiny_loss[k] / max(abs(float(r[k])), 1e-300), (name, lam, k, got_loss[k], float(r[k]), e_loss[k], fl[k])


PAIRS = ['one_frame_short', 'empty_and_short', 'tgt_len_guard', 'waves_v50', 'straddle_on', 'ragged_in_len', 'blank_mid', 'peaked_x4']


@pytest.mark.parametrize('lam', [0.3, 0.5])
@pytest.mark.parametrize('name', PAIRS)
def test_ctc_pair_matches_float64(name, lam):
    loss3, nll, g = run_pair(name, lam)
    check_pair_against_reference(name, lam, loss3, nll, g)
    only = run_pair(name, lam, grad=False)                               # dlogits == NULL: the same losses, no atomics anywhere
    assert torch.equal(only[0], loss3) and torch.equal(only[1], nll)
    again = run_pair(name, lam)
    assert torch.equal(again[0], loss3) and torch.equal(again[1], nll)


def _same_slab(name, p, ga, gb, tag):
    """two launches that must give utterance p the same slab: the bound tests/test_gpu_ctc_loss.py uses between two runs"""
    tn = cc.tiny_of(name)
    d, n = float((ga[p].double() - gb[p].double()).norm()), float(ga[p].double().norm())
    assert d <= 2 * float(tn[p]) * n, (name, tag, 'utterance %d' % p, d / max(n, 1e-300))


@pytest.mark.parametrize('name', ['one_frame_short', 'empty_and_short', 'tgt_len_guard'])
def test_an_infeasible_set_leaves_its_partner_and_its_neighbours_alone(name):
    """the same pair with the infeasible / guarded entries made feasible (raised_in_len: the frames, shared by both sets;
    raised_tgt_len: one set's target length, the partner stays as it was).  Before: nll exactly 0, the slab the other set's gradient
    alone (checked against float64 by test_ctc_pair_matches_float64) or exactly zero.  After: only the raised utterances change."""
    lam = 0.3
    a, b = ref.pair_of(name)
    P = a['logits'].shape[0]
    feas = (cc.feasible(a), cc.feasible(b))
    base = run_pair(name, lam)
    for p in range(P):
        for k in (0, 1):
            if not feas[k][p]:
                assert float(base[1][k, p]) == 0.0, (name, p, k)
        if not (feas[0][p] or feas[1][p]):
            assert float(base[2][p].abs().max()) == 0.0, (name, p)
    runs = []
    if a['raised_in_len'] is not None:
        changed = [p for p in range(P) if int(a['raised_in_len'][p]) != int(a['in_len'][p])]
        runs.append(('raised_in_len', dict(in_len=a['raised_in_len']), changed, None))
    if a.get('raised_tgt_len') is not None:
        changed = [p for p in range(P) if int(a['raised_tgt_len'][p]) != int(a['tgt_len'][p])]
        runs.append(('raised_tgt_len of set a', dict(tgt_len_a=a['raised_tgt_len']), changed, 1))
        changed = [p for p in range(P) if int(b['raised_tgt_len'][p]) != int(b['tgt_len'][p])]
        runs.append(('raised_tgt_len of set b', dict(tgt_len_b=b['raised_tgt_len']), changed, 0))
    assert runs
    for tag, kw, changed, partner in runs:
        assert changed
        got = run_pair(name, lam, **kw)
        for p in range(P):
            if p not in changed:
                assert torch.equal(got[1][:, p], base[1][:, p]), (name, tag, p)
                _same_slab(name, p, base[2], got[2], tag)
            elif partner is not None:                                    # the partner set of a raised utterance keeps its nll bit for bit
                assert torch.equal(got[1][partner, p], base[1][partner, p]), (name, tag, p)
        raised_set = {None: (0, 1), 1: (0,), 0: (1,)}[partner]
        moved = [p for p in changed if any(not feas[k][p] for k in raised_set)]
        assert moved
        for p in moved:                                                  # and it is the length that did it
            assert any(float(got[1][k, p]) > 0.0 and float(base[1][k, p]) == 0.0 for k in raised_set), (name, tag, p)
            assert float((got[2][p] - base[2][p]).abs().max()) > 0.0, (name, tag, p)


@pytest.mark.parametrize('lam', [1.0, 0.0])
@pytest.mark.parametrize('name', ['waves_v50', 'one_frame_short'])
def test_weight_one_is_otr_ctc_loss_on_that_set_alone(name, lam):
    """lam = 1: loss, loss_a, nll row a and the gradient are otr_ctc_loss's on set a (nll bit-equal, slabs within 2 tiny of each other,
    the bounds tests/test_gpu_ctc_loss.py uses for two runs of that kernel); lam = 0 the mirror image.  The other set is poisoned: its
    labels and target lengths are tgt_len_guard's (lengths of 41, 127, 10 ** 6 and -1 among them), which must not leak at weight 0."""
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    c = cc.build(name)
    guard = cc.build('tgt_len_guard')
    P, T, V = c['logits'].shape
    W = c['targets'].shape[1]
    poison_t = torch.ones((P, W), dtype=torch.int64)
    w = min(W, guard['targets'].shape[1])
    rows = [p % guard['targets'].shape[0] for p in range(P)]
    poison_t[:, :w] = guard['targets'][rows, :w]
    poison_l = guard['tgt_len'][rows]
    keep = 0 if lam == 1.0 else 1
    sets = [(c['targets'], c['tgt_len']), (poison_t, poison_l)]
    if keep == 1:
        sets.reverse()
    lp = ops.log_softmax(c['logits'].to(DEV))
    both = torch.stack((sets[0][0], sets[1][0]), dim=1).reshape(2 * P, W).to(DEV)
    i32 = lambda t: t.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(DEV)    # noqa: E731
    ws = torch.full((2, P, T, 2 * W + 1), float('nan'), dtype=torch.float32, device=DEV)
    nll = torch.full((2, P), -7.0, dtype=torch.float32, device=DEV)
    loss3 = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    dl = torch.full((P, T, V), -7.0, dtype=torch.float32, device=DEV)
    la, lb, il, lam_d = i32(sets[0][1]), i32(sets[1][1]), i32(c['in_len']), _lam_dev(lam)       # named: alive until the launch has run
    L.check(L.load().otr_ctc_loss_pair(_p(lp), _p(both[0::2]), 2 * W, _p(la), _p(both[1::2]), 2 * W, _p(lb), _p(il), _p(lam_d), P, T, V, W,
                                       c['blank'], _p(ws), _p(nll), _p(loss3), _p(dl), _stream()), 'otr_ctc_loss_pair')
    torch.cuda.synchronize()
    single = run_direct(c)
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(loss3).all())
    check_same_result(name, 'lam = %g against otr_ctc_loss' % lam, single, (None, nll[keep], dl))
    for got in (loss3[0], loss3[1 + keep]):                               # an ordered sum here, an atomic one there: P additions apart
        assert abs(float(got) - float(single[0])) <= P * cc.EPS32 * abs(float(single[0])), (name, lam, float(got), float(single[0]))


def test_ops_ctc_loss_pair_through_autograd():
    """the autograd function: one gradient, scaled by the incoming seed in backward; loss_a and loss_b are detached"""
    from opentransformer_amd import ops
    name, lam = 'ragged_in_len', 0.3
    a, b = ref.pair_of(name)
    x = a['logits'].to(DEV).requires_grad_(True)
    args = (a['targets'].to(DEV), b['targets'].to(DEV), a['in_len'].to(DEV), a['tgt_len'].to(DEV), b['tgt_len'].to(DEV), _lam_dev(lam), a['blank'])
    loss, loss_a, loss_b = ops.ctc_loss_pair(x, *args)
    assert loss.requires_grad and not loss_a.requires_grad and not loss_b.requires_grad
    (g,) = torch.autograd.grad(3.0 * loss, x)
    direct = run_pair(name, lam)
    assert torch.equal(loss.detach(), direct[0][0]) and torch.equal(loss_a, direct[0][1]) and torch.equal(loss_b, direct[0][2])
    for p in range(x.shape[0]):
        _same_slab(name, p, 3.0 * direct[2], g, 'autograd, seed 3')
    only = ops.ctc_loss_pair(a['logits'].to(DEV), *args)                 # logits without a gradient: the loss-only path
    assert not only[0].requires_grad and torch.equal(only[0], loss.detach())


# ------------------------------------------------------------------------------------------ model level
LAM = 0.3
BATCH = dict(batch=5, frames=96, feat_dim=80, vocab=100, tgt_len=6, seed=5, lengths=[96, 80, 96, 64, 50], tgt_lengths=[6, 4, 5, 6, 3])


def _cfg(kind):
    cfg = syn.c1_model(0.0, ctc_weight=0.3 if kind == 'joint' else 0.0)
    return dict(cfg, vocab_size=cfg['decoder']['vocab_size']) if kind == 'ctc' else cfg


def _model_case(mode, kind):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ops.set_compute_dtype(mode)
    cfg = _cfg(kind)
    model = (ota.CTCModel if kind == 'ctc' else ota.SpeechToText)(cfg)
    syn.fill_state_dict_(model.state_dict(), 1234)
    inputs, targets = syn.synthetic_batch(**BATCH)
    to_dev = lambda d: {k: v.to(DEV) for k, v in d.items()}              # noqa: E731
    return model.to(DEV).train(), to_dev(inputs), to_dev(targets), cfg


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """the CPU oracle composite on BATCH at LAM, once per kind: (loss, loss_1, loss_2, {parameter name: gradient})"""
    cfg = _cfg(kind)
    inputs, targets = syn.synthetic_batch(**BATCH)
    loss, loss_1, loss_2, parts = ref.oracle_composite(cfg, inputs, targets, LAM, kind=kind)
    loss.backward()
    return loss.item(), loss_1.item(), loss_2.item(), {k: v.grad for k, v in H.flat_named(parts).items() if v.grad is not None}


def _fault_counter():
    from opentransformer_amd import ops
    fault = ops.fault_counter(torch.device(DEV, torch.cuda.current_device()))
    fault.zero_()
    return fault


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _summary_err(key, got, want):
    """the measure TOL16's gradient bar belongs to (tests/test_gpu_model.py::run_train_case): the larger of the norm's and the probe
    dot's distance from the reference's, relative to the reference norm"""
    a, b = got.double().reshape(-1).cpu().numpy(), want.double().reshape(-1).numpy()
    probe = H.probe_vector(key, b.size)
    nrm = np.sqrt((b * b).sum())
    return max(abs(np.sqrt((a * a).sum()) - nrm) / max(nrm, 1e-4),
               abs((a * probe).sum() - (b * probe).sum()) / max(nrm * np.sqrt(b.size), 1e-4 * np.sqrt(b.size)))


@pytest.mark.parametrize('kind', ['att', 'joint', 'ctc'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_training_step_matches_the_cpu_oracle_composite(mode, kind):
    """loss and parameter gradients against lam * oracle(mixed, t1) + (1 - lam) * oracle(mixed, t2); fp32: loss 1e-4 and gradients 2e-3
    relative (tests/test_gpu_model.py::test_c1_fp32_matches_cpu_oracle_on_fresh_inputs), bf16: TOL16['bf16'] (loss, worst gradient)"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, _ = _model_case(mode, kind)
        fault = _fault_counter()
        wrap = ota.MixSpeechTraining(model).train()
        loss, aux = wrap(inputs, targets, lam=LAM)
        ops.backward(loss)
        torch.cuda.synchronize()
        want, want_1, want_2, want_g = _oracle(kind)
        tol_loss, tol_grad = (1e-4, 2e-3) if mode == 'fp32' else (TOL16['bf16'][0], TOL16['bf16'][2])
        assert sorted(aux) == sorted(['Lambda', 'Loss_1', 'Loss_2'] + (['CTCLoss'] if kind != 'att' else []))
        assert float(aux['Lambda']) == float(np.float32(LAM)) and not any(v.requires_grad for v in aux.values())
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        if mode == 'fp32':
            errs = {k: _rel(g.cpu(), want_g[k]) for k, g in grads.items() if float(want_g[k].norm()) > 1e-6}
        else:
            errs = {k: _summary_err(k, g, want_g[k]) for k, g in grads.items()}
        worst = max(errs, key=errs.get)
        print('mixspeech %s %s: loss %.7f oracle %.7f, Loss_1 %.7f / %.7f, Loss_2 %.7f / %.7f, worst gradient %s %.3g' % (
            mode, kind, loss.item(), want, float(aux['Loss_1']), want_1, float(aux['Loss_2']), want_2, worst, errs[worst]))
        assert len(grads) > 10 and set(grads) <= set(want_g)
        for got, ref_v in ((loss.item(), want), (float(aux['Loss_1']), want_1), (float(aux['Loss_2']), want_2)):
            assert abs(got - ref_v) < tol_loss * abs(ref_v), (got, ref_v)
        for k, e in errs.items():
            assert e < tol_grad, (k, e)
        assert int(fault.item()) == 0
    finally:
        ops.set_compute_dtype('bf16')


def test_the_dropped_utterance_has_no_influence():
    """B = 5: the fifth utterance takes no part; other features, another length and other targets there leave the loss bit-equal"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, _ = _model_case('fp32', 'att')
        fault = _fault_counter()
        wrap = ota.MixSpeechTraining(model).train()
        lam = _lam_dev(LAM)
        with torch.no_grad():
            base, _ = wrap(inputs, targets, lam=lam)
            inputs2 = {k: v.clone() for k, v in inputs.items()}
            targets2 = {k: v.clone() for k, v in targets.items()}
            inputs2['inputs'][4] = 3.0
            inputs2['inputs_length'][4] = 96
            inputs2['mask'][4] = True
            targets2['targets'][4, 1:4] = 7
            other, _ = wrap(inputs2, targets2, lam=lam)
        assert torch.equal(base, other)
        assert int(fault.item()) == 0
    finally:
        ops.set_compute_dtype('bf16')


def test_eval_returns_the_plain_model():
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, _ = _model_case('fp32', 'att')
        fault = _fault_counter()
        wrap = ota.MixSpeechTraining(model).eval()
        with torch.no_grad():
            got, aux = wrap(inputs, targets)
            want, want_aux = model(inputs, targets)
        assert torch.equal(got, want) and aux is None and want_aux is None
        assert int(fault.item()) == 0
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('kind', ['att', 'joint', 'ctc'])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_identical_pairs_give_the_plain_step_of_the_even_half(mode, kind):
    """inputs[2p + 1] == inputs[2p] and equal targets in every pair, lam = 0.5 (0.5 x + 0.5 x is x exactly): both target sets are one and
    the loss is the plain loss of the even half batch.  Bound: the one tests/test_gpu_distill.py::test_kd_weight_zero_is_the_plain_step
    uses between two passes -- bit-equal without a CTC head, 4 * 2^-23 relative with one (otr_ctc_loss adds its terms with
    floating-point atomics, the pair call in utterance order)."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, _ = _model_case(mode, kind)
        fault = _fault_counter()
        twin = lambda d: {k: v[[0, 0, 2, 2]].contiguous() for k, v in d.items()}      # noqa: E731
        half = lambda d: {k: v[[0, 2]].contiguous() for k, v in d.items()}            # noqa: E731
        wrap = ota.MixSpeechTraining(model).train()
        with torch.no_grad():
            got, aux = wrap(twin(inputs), twin(targets), lam=0.5)
            plain, _ = model(half(inputs), half(targets))
        print('mixspeech identical pairs %s %s: loss %.9g plain %.9g' % (mode, kind, got.item(), plain.item()))
        bound = 0.0 if kind == 'att' else 4 * 2.0 ** -23 * abs(plain.item())
        assert abs(got.item() - plain.item()) <= bound
        assert float(aux['Loss_1']) == float(aux['Loss_2'])
        assert int(fault.item()) == 0
    finally:
        ops.set_compute_dtype('bf16')


def test_hipgraph_replay_reads_lambda_and_the_batch_from_the_device():
    """forward + backward of the joint case captured once (the pattern of tests/test_gpu_model.py::test_hipgraph_replay_matches_eager);
    the lam buffer and the input batch are then overwritten in place, and the replay must be the eager step on the new values"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel
    ops.set_compute_dtype('bf16')
    model, inputs, targets, _ = _model_case('bf16', 'joint')
    fault = _fault_counter()
    wrap = ota.MixSpeechTraining(model).train()
    dp = FlatDataParallel(wrap)
    lam = wrap.set_lambda(LAM, inputs['inputs'].device)
    out = {}

    def fwd_bwd():
        dp.zero_grad()
        loss, _ = dp(inputs, targets, lam=lam)
        loss.backward()
        out['loss'] = loss.detach()

    fwd_bwd()
    torch.cuda.synchronize()
    first = dp.flat_grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        fwd_bwd()
    captured = out['loss']
    # new values, in place: another lam and another batch (the same shapes and lengths)
    fresh, _ = syn.synthetic_batch(**dict(BATCH, seed=11))
    inputs['inputs'].copy_(fresh['inputs'].to(DEV))
    lam.fill_(0.8)
    dp.flat_grad.fill_(float('nan'))
    g.replay()
    torch.cuda.synchronize()
    replay_loss, replay_grad = float(captured), dp.flat_grad.clone()
    fwd_bwd()
    torch.cuda.synchronize()
    eager_loss, eager_grad = float(out['loss']), dp.flat_grad.clone()
    assert bool(torch.isfinite(replay_grad).all())
    rel = _rel(replay_grad, eager_grad)
    print('mixspeech graph replay: loss %.7f eager %.7f, gradient rel %.3g; against the captured values rel %.3g' % (
        replay_loss, eager_loss, rel, _rel(replay_grad, first)))
    assert abs(replay_loss - eager_loss) <= 1e-5 * abs(eager_loss)
    assert rel < 1e-4                                                    # atomics reorder the last ulps
    assert _rel(replay_grad, first) > 1e-2                               # and the replay did read the new values
    assert int(fault.item()) == 0
