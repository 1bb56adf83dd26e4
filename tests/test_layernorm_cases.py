"""CPU: the LayerNorm cases of tests/layernorm_cases.py are what their names claim and together cover the shapes, families and options
the kernels branch on; the float64 reference agrees with torch's float64 LayerNorm and its autograd; floor() -- the emulated working
precision, in three summation orders -- stays at or below half of the per-element bounds on every case in both modes; every mutant
leaves them on at least one named case: a failure of tests/test_gpu_layernorm.py is the kernel's, and a pass means something."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import layernorm_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r'^(fwd|bwd|fwd2|bwd2|fwd3|bwd3)_d(\d+)nv(\d)([te])_M(\d+)q(\d)o(\d)_([fh])_([a-z]+)(?:_(.+))?$')


def _all(mode='bf16'):
    return [lc.realise(n, mode) for n in lc.NAMES]


def test_every_case_is_what_its_name_claims():
    assert len(set(lc.NAMES)) == len(lc.NAMES) > 200
    for c in _all():
        m = NAME.match(c['name'])
        assert m, c['name']
        entry, d, nv, tail, M, q, o, at, fam, _ = m.groups()
        d, M = int(d), int(M)
        assert (entry, d, M, at, fam) == (c['entry'], c['d'], c['M'], c['at'], c['family'])
        assert d % 4 == 0 and d <= 1024 and M * d <= 17 * 1024
        slots = -(-d // 256)                                   # float4 slots per lane; the last one is partial when d is no multiple of 256
        lanes_in_tail = (d - (slots - 1) * 256) // 4 % 64
        assert (int(nv), tail == 't') == (slots, lanes_in_tail != 0), c['name']
        assert lc.D_TABLE[d] == (slots, lanes_in_tail) and lc.M_TABLE[M] == (M % 4, M % 8) == (int(q), int(o)), c['name']
        assert c['C'] == 4 * slots + 10 and c['nblk'] == -(-M // 8)
        assert fam in lc.FAMILIES and c['mask'] == (fam == 'masked')
        if c['entry'] in ('bwd2', 'bwd3'):
            assert c['partial']                                # those entries have no atomics path


def test_the_cases_cover_the_design():
    cs = _all()
    have = lambda **kw: [c for c in cs if all(c[k] == v for k, v in kw.items())]
    fwd, bwd = ('fwd', 'fwd2', 'fwd3'), ('bwd', 'bwd2', 'bwd3')
    for d in lc.D_TABLE:                                       # every d with M = 1 and M = 9, forward and backward
        for M in (1, 9):
            assert any(c['entry'] in fwd for c in have(d=d, M=M)) and any(c['entry'] in bwd for c in have(d=d, M=M)), (d, M)
    for M in lc.M_TABLE:                                       # every M with d = 260 and d = 1024
        for d in (260, 1024):
            assert have(d=d, M=M, entry='fwd') and have(d=d, M=M, entry='bwd') and have(d=d, M=M, entry='bwd3'), (d, M)
    for nv in (1, 2, 3, 4):                                    # every NV with every form and both `a` types
        for e in lc.ENTRIES:
            for at in 'fh':
                assert [c for c in have(entry=e, at=at) if lc.D_TABLE[c['d']][0] == nv], (nv, e, at)
    for f in lc.FAMILIES:
        for e in lc.ENTRIES:
            assert have(family=f, entry=e), (f, e)
    for p in (0.1, 0.5):                                       # the options
        for e in ('fwd', 'bwd', 'bwd2', 'bwd3'):
            assert any(c['rng_offset'] != 0 for c in have(p=p, entry=e)), (p, e)
    assert lc.SEED >> 32 != 0 and have(rng_offset=lc.RNG_OFFSET_BIG)
    assert have(a_scale=0.0, entry='bwd') and have(a_scale=0.5, entry='bwd') and have(a_scale=0.5, entry='fwd')
    for part in (False, True):
        assert have(entry='bwd', partial=part, dy16=True) and have(entry='bwd', partial=part, has_a=False)
        assert have(entry='bwd', partial=part, skip='alias') and have(entry='bwd', partial=part, family='masked', p=0.1)
    assert have(entry='bwd3', dy3_16=True) and have(entry='bwd3', dy3_16=False)
    for e in bwd:
        assert {c['skip'] for c in have(entry=e)} == {'none', 'sep', 'alias'}, e
        assert have(entry=e, has_a=False)
    assert have(entry='fwd', lp_only=True) and have(entry='fwd3', lp_only=True) and have(entry='fwd', z_out=False)
    for e in fwd:
        assert have(entry=e, has_a=False)


def test_no_case_is_skipped():
    """the GPU module runs every case in both modes: nothing is dropped between the list here and its parametrisation"""
    from tests import test_gpu_layernorm as tg
    assert sorted(tg.CASES) == sorted((m, n) for m in lc.MODES for n in lc.NAMES)


def test_the_dropout_mask_is_the_hash_the_tool_restates():
    spec = importlib.util.spec_from_file_location('dropout_hash_check', os.path.join(ROOT, 'tools', 'dropout_hash_check.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    idx = np.uint64(lc.RNG_OFFSET_BIG - 4000) + np.arange(8000, dtype=np.uint64)          # across the index's 2^32 boundary
    assert np.array_equal(lc.rand32(lc.SEED, idx), tool.rand32(lc.SEED, idx))
    for p, thr in ((0.1, 429496736), (0.5, 2147483648)):       # uint32(float32(p) * 2^32): float32(0.1) is a little above 0.1
        c = dict(M=17, d=1024, p=p, rng_offset=lc.RNG_OFFSET)
        keep = lc.keep_mask(c)
        assert np.array_equal(keep.ravel(), lc.rand32(lc.SEED, np.uint64(lc.RNG_OFFSET) + np.arange(17 * 1024, dtype=np.uint64)) >= thr)
        assert abs(keep.mean() - (1 - p)) < 4 * (p * (1 - p) / keep.size) ** 0.5
    assert lc.branch_scale(dict(p=0.1, a_scale=0.5)) == np.float32(np.float32(1) / np.float32(0.9) * np.float32(0.5))
    assert lc.branch_scale(dict(p=0.0, a_scale=0.0)) == 1.0


@pytest.mark.parametrize('name', ['fwd3_d1020nv4t_M17q1o1_h_masked', 'fwd3_d260nv2t_M7q3o7_f_unit_p1_bigoff', 'fwd_d516nv3t_M9q1o1_h_unit_p5'])
def test_forward_reference_against_torch_float64(name):
    c = lc.realise(name, 'fp16')
    o = lc.operands(c)
    ref = lc.reference(c)
    t = lambda k: torch.from_numpy(o[k]).double()
    a = torch.where(torch.from_numpy(o['amask'] != 0)[:, None], t('a'), torch.zeros(())) if o['amask'] is not None else t('a')
    z = t('x') + float(lc.branch_scale(c)) * torch.from_numpy(lc.keep_mask(c)).double() * a
    F = torch.nn.functional
    y = z
    for k in '123'[:int(c['entry'][3:] or 1)]:
        y = F.layer_norm(y, (c['d'],), t('gamma' + k), t('beta' + k), float(np.float32(lc.EPS)))
    last = 'y3' if c['entry'] == 'fwd3' else 'y'
    assert np.abs(ref['z'][0] - z.numpy()).max() < 1e-12 and np.abs(ref[last][0] - y.numpy()).max() < 1e-10
    assert np.isfinite(ref[last][0]).all() and np.isfinite(ref[last][1]).all()


@pytest.mark.parametrize('name', ['bwd_d260nv2t_M9q1o1_h_masked_p1_atom', 'bwd2_d260nv2t_M9q1o1_f_unit_p5', 'bwd3_d772nv4t_M9q1o1_h_unit_p1',
                                  'bwd3_d260nv2t_M17q1o1_f_unit_dy3h_alias'])
def test_backward_reference_against_torch_autograd(name):
    """the chained analytic gradient is autograd's; the case's statistics are float64 values rounded to fp32 and autograd's are exact,
    which is worth 2^-24 relative: compared at 1e-5 of the largest element"""
    c = lc.realise(name, 'bf16')
    o = lc.operands(c)
    ref = lc.reference(c)
    d = c['d']
    t = lambda k: torch.from_numpy(o[k]).double()
    z = t('z').requires_grad_(True)
    ps = [t(k + i).requires_grad_(True) for i in '123' for k in ('gamma', 'beta')]
    F = torch.nn.functional
    eps = float(np.float32(lc.EPS))
    y1 = F.layer_norm(z, (d,), ps[0], ps[1], eps)
    y2 = F.layer_norm(y1, (d,), ps[2], ps[3], eps)
    y3 = F.layer_norm(y2, (d,), ps[4], ps[5], eps)
    outs, gs = {'bwd': ([y1], [t('dy')]), 'bwd2': ([y2], [t('dy')]), 'bwd3': ([y2, y3], [t('dy'), t('dy3')])}[c['entry']]
    if o['skip'] is not None:
        outs, gs = outs + [z], gs + [t('skip')]
    n = {'bwd': 2, 'bwd2': 4, 'bwd3': 6}[c['entry']]
    g = torch.autograd.grad(outs, [z] + ps[:n], gs)
    rowm = (o['amask'] != 0)[:, None] if o['amask'] is not None else True
    sc = np.where(lc.keep_mask(c) & rowm, float(lc.branch_scale(c)), 0.0)
    want = {'dx': g[0].numpy(), 'da': g[0].numpy() * sc, 'dacol': (g[0].numpy() * sc).sum(0)}
    for i, k in enumerate(('dgamma', 'dbeta', 'dgamma2', 'dbeta2', 'dgamma3', 'dbeta3')[:n]):
        want[k] = g[1 + i].numpy()
    for k, w in want.items():
        r = ref[k][0]
        if k in ('dgamma', 'dbeta', 'dacol') and not c['partial']:
            r = r - lc.prior(d, ('dgamma', 'dbeta', 'dacol').index(k))
        assert np.abs(r - w).max() < 1e-5 * max(np.abs(w).max(), 1.0), (k, np.abs(r - w).max())


@pytest.mark.parametrize('mode', lc.MODES)
@pytest.mark.parametrize('order', lc.ORDERS)
def test_floor_stays_within_half_the_bound(mode, order):
    over = []
    for c in _all(mode):
        w = lc.floor(c, order)
        if not w[0] <= 0.5:
            over.append((c['name'],) + w)
        w16 = lc.floor(c, order, round16=True)                 # ... and with the 16-bit-only outputs rounded, inside the whole bound
        assert w16[0] <= 1.0, (c['name'],) + w16
    assert not over, '%d cases above 0.5 of the bound, e.g. %r' % (len(over), over[:5])


@pytest.mark.parametrize('mutant', lc.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    hits = [c['name'] for c in _all() if lc.mutant_ratio(c, mutant)[0] > 1.0]
    assert hits, mutant
    if mutant == 'mask_mul':                                   # fed Inf / NaN in a masked row: every forward case of the family
        assert set(hits) == {c['name'] for c in _all() if c['family'] == 'masked' and c['entry'][0] == 'f'}
    if mutant == 'phantom':                                    # only where the last workgroup has rows past M
        assert all(lc.CASES[n]['M'] % 8 for n in hits)


def test_the_bounds_are_finite_and_positive():
    for mode in lc.MODES:
        for c in _all(mode):
            for k, (r, b) in lc.reference(c).items():
                assert np.isfinite(r).all() and np.isfinite(b).all() and (b >= 0).all(), (c['name'], k)
