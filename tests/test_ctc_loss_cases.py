"""CPU (-m "not gpu"): every case of tests/ctc_loss_cases.py is what its name says, judged from the float64 reference alone, so
that tests/test_gpu_ctc_loss.py cannot pass (or fail) on a mislabelled case."""
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_loss_cases as cc


def _raw_nll(c):
    """float64 nll without zero_infinity: inf where no alignment exists"""
    T = c['logits'].shape[1]
    il, tl, _ = cc.effective_lengths(c['targets'], c['in_len'], c['tgt_len'], T)
    lp = F.log_softmax(c['logits'].double(), -1).transpose(0, 1)
    return F.ctc_loss(lp, c['targets'], il, tl, blank=c['blank'], reduction='none', zero_infinity=False)


@pytest.mark.parametrize('name', cc.NAMES)
def test_case_is_what_it_claims(name):
    c = cc.build(name)
    B, T, V = c['logits'].shape
    W = c['targets'].shape[1]
    assert c['logits'].dtype == torch.float32 and c['targets'].dtype == torch.int64 and W <= 127
    assert 0 <= c['blank'] < V and int(c['targets'].min()) >= 0 and int(c['targets'].max()) < V
    il, tl, guarded = cc.effective_lengths(c['targets'], c['in_len'], c['tgt_len'], T)
    for b in range(B):                                      # no label inside a target is the blank
        assert not bool((c['targets'][b, :int(tl[b])] == c['blank']).any()), b
    loss, nll, g = cc.reference_of(name)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(nll).all()) and bool(torch.isfinite(g).all())
    # feasibility: T_b >= L_b + repeats_b, seen by the reference as a finite nll
    feas = cc.feasible(c)
    raw = _raw_nll(c)
    for b in range(B):
        if int(il[b]) >= 1 and not bool(guarded[b]):
            assert bool(torch.isfinite(raw[b])) == feas[b], (b, float(raw[b]))
        if feas[b]:
            assert float(nll[b]) > 0.0 and float(g[b].abs().max()) > 0.0, b
            assert float(g[b, int(il[b]):].abs().max() if int(il[b]) < T else 0.0) == 0.0, b
        else:
            assert float(nll[b]) == 0.0 and float(g[b].abs().max()) == 0.0, b
    assert guarded.nonzero().flatten().tolist() == c['guarded']
    assert set(c['infeasible']) <= {b for b in range(B) if not feas[b] and not bool(guarded[b])}
    assert all(feas[b] for b in c['single_path'])
    # the mean the kernel documents: mean_b(nll_b / max(L_b, 1))
    assert abs(float(loss) - float((nll / tl.clamp_min(1)).mean())) <= 1e-12 * abs(float(loss))
    fl = cc.floor_of(name)
    assert all(bool(torch.isfinite(fl[k]).all()) for k in ('nll', 'grad', 'rowsum')) and fl['loss'] == fl['loss']
    tn = cc.tiny_of(name)
    assert bool(torch.isfinite(tn).all()) and all(float(tn[b]) > 0 for b in range(B) if feas[b])
    assert float(tn.max()) < 5e-3          # the slack stays a rounding-sized term at every shape used


@pytest.mark.parametrize('name', ['waves_v50', 'waves_v4233', 'blank_last', 'blank_mid'])
def test_wave_cases_reach_every_boundary(name):
    c = cc.build(name)
    assert c['tgt_len'].tolist() == cc.WAVE_LENGTHS and c['logits'].shape[1] >= 2 * 127 + 1
    last = [2 * L for L in c['tgt_len'].tolist()]                      # last live state, S - 1
    assert [s // 64 for s in last] == [0, 1, 1, 1, 2, 2, 2, 3, 3]      # 62 | 64 66, 126 | 128 130, 190 | 192, 254
    assert {63, 64, 65}.issubset({L for L in c['tgt_len'].tolist()}) and max(last) == 254
    assert all(cc.feasible(c))
    assert c['blank'] == {'waves_v50': 0, 'waves_v4233': 0, 'blank_last': 49, 'blank_mid': 25}[name]
    assert c['logits'].shape[2] == (4233 if name == 'waves_v4233' else 50)


@pytest.mark.parametrize('name,off', [('straddle_before', -1), ('straddle_on', 0), ('straddle_after', 1)])
def test_straddle_cases_have_the_pair_at_the_stated_states(name, off):
    c = cc.build(name)
    want = {0: [(63, 65), (127, 129), (191, 193)], -1: [(61, 63), (125, 127), (189, 191)], 1: [(65, 67), (129, 131), (193, 195)]}[off]
    seen = set()
    for b, at in c['repeat_at'].items():
        L = int(c['tgt_len'][b])
        r = c['targets'][b, :L]
        pairs = [(2 * i + 1, 2 * i + 3) for i in range(L - 1) if int(r[i]) == int(r[i + 1])]      # every repeat of the target
        assert pairs == [(2 * i + 1, 2 * i + 3) for i in at] and all(p in want for p in pairs), (b, pairs)
        for lo, hi in pairs:
            assert (lo // 64 != hi // 64) == (off == 0)          # across a wave boundary only in straddle_on
            assert hi + 1 < 2 * L + 1                            # the state after the pair is live
        seen.update(pairs)
    assert seen == set(want)
    assert cc.repeats(c) == [len(c['repeat_at'][b]) for b in range(len(c['repeat_at']))]
    assert all(cc.feasible(c))


def test_single_path_equals_the_closed_form():
    c = cc.build('single_path')
    loss, nll, g = cc.reference_of('single_path')
    assert c['single_path'] == [0, 2] and [int(c['tgt_len'][b]) for b in (0, 2)] == [40, 100]
    for b in c['single_path']:
        L = int(c['tgt_len'][b])
        assert int(c['in_len'][b]) == 2 * L - 1 and bool((c['targets'][b, :L] == c['targets'][b, 0]).all())
        want_nll, want_g = cc.single_path_closed_form(c, b)
        assert abs(float(nll[b] - want_nll)) <= 1e-12 * float(want_nll), b
        assert float((g[b] - want_g).abs().max()) <= 1e-12, b


def test_one_frame_short_has_no_alignment_and_leaves_the_neighbours_alone():
    c, full = cc.build('one_frame_short'), cc.build('single_path')
    assert c['infeasible'] == [0, 2] and cc.feasible(c) == [False, True, False, True]
    assert torch.equal(c['logits'], full['logits']) and torch.equal(c['targets'], full['targets'])
    assert (full['in_len'] - c['in_len']).tolist() == [1, 0, 1, 0] and torch.equal(c['raised_in_len'], full['in_len'])
    _, nll, g = cc.reference_of('one_frame_short')
    _, nll_full, g_full = cc.reference_of('single_path')
    for b in (1, 3):
        assert float(nll[b]) == float(nll_full[b]) and torch.equal(g[b], g_full[b])
    assert bool(torch.isinf(_raw_nll(c)[[0, 2]]).all())


def test_degenerate_lengths():
    c = cc.build('empty_and_short')
    T = c['logits'].shape[1]
    assert list(zip(c['tgt_len'].tolist(), c['in_len'].tolist())) == [(0, T), (100, T), (5, 0), (0, 0), (0, 1), (1, 1), (2, 1), (127, 205)]
    assert cc.feasible(c) == [True, True, False, False, True, True, False, True]
    lp = F.log_softmax(c['logits'].double(), -1)
    _, nll, g = cc.reference_of('empty_and_short')
    assert abs(float(nll[0] + lp[0, :, 0].sum())) <= 1e-9                       # L = 0: blanks all the way
    assert abs(float(nll[4] + lp[4, 0, 0])) <= 1e-12 and abs(float(nll[5] + lp[5, 0, int(c['targets'][5, 0])])) <= 1e-12
    cf = cc.coef(c['tgt_len'], c['targets'], 8)
    assert cf.tolist() == [1 / 8, 1 / 800, 1 / 40, 1 / 8, 1 / 8, 1 / 8, 1 / 16, 1 / (8 * 127)]      # max(L, 1)
    want = lp[4, 0].exp()
    want[0] -= 1.0
    assert float((g[4, 0] - want * cf[4]).abs().max()) <= 1e-15
    raised = dict(c, in_len=c['raised_in_len'])
    assert cc.feasible(raised) == [True, True, True, False, True, True, True, True]


def test_length_edge_cases():
    c = cc.build('ragged_in_len')
    T = c['logits'].shape[1]
    assert int((c['in_len'] < T).sum()) >= 6 and int((c['in_len'] == T).sum()) >= 1 and all(cc.feasible(c))
    c = cc.build('in_len_clamp')
    T = c['logits'].shape[1]
    assert int((c['in_len'] > T).sum()) == 3 and torch.equal(c['clamped_in_len'], c['in_len'].clamp(max=T))
    assert int(c['in_len'].max()) == 2 ** 31 - 1 and all(cc.feasible(c))
    c = cc.build('tgt_len_guard')
    W = c['targets'].shape[1]
    assert W == 40 and c['guarded'] == [1, 3, 4, 5]
    for b in c['guarded']:                       # the kernel's guard `L < 0 || 2 L + 1 > Smax` with Smax = 2 W + 1 is what refuses them
        L = int(c['tgt_len'][b])
        assert L < 0 or 2 * L + 1 > 2 * W + 1
    assert W + 1 in c['tgt_len'].tolist() and 127 in c['tgt_len'].tolist() and -1 in c['tgt_len'].tolist()
    assert 2 * W + 1 <= 256 and int(c['tgt_len'].max()) < 2 ** 30           # the entry's own width check passes; 2 L + 1 fits int32
    assert all(cc.feasible(dict(c, tgt_len=c['raised_tgt_len'])))


def test_large_cases_have_the_stated_shapes():
    for name, scale in (('peaked_x4', 4.0), ('peaked_x8', 8.0)):
        c = cc.build(name)
        assert tuple(c['logits'].shape) == (4, 349, 4233) and abs(float(c['logits'].std()) - scale) < 0.05 * scale
        assert c['tgt_len'].tolist() == [44, 100, 127, 10] and all(cc.feasible(c))
    c = cc.build('aishell')
    assert tuple(c['logits'].shape) == (32, 250, 4233)
    assert int(c['tgt_len'].min()) == 1 and int(c['tgt_len'].max()) == 44 and int((2 * c['tgt_len'] + 1 > 64).sum()) >= 4
    assert int((c['in_len'] < 250).sum()) >= 16 and all(cc.feasible(c))
