"""CPU: the GEMM cases of tests/gemm_cases.py are what they claim (plan() replays gemm_launch_tiles of csrc/gemm_kernel.h), together
they reach every path of the launcher, floor() -- the emulated working precision -- stays inside the per-element bound on every case
in every mode, and every mutant of the expected result leaves it: a failure of tests/test_gpu_gemm.py is the kernel's, and a pass
means something."""
import pytest
import torch

from tests import gemm_cases as gc

ALL = [(m, n) for m in gc.MODES for n in gc.names_for(m)]
SMALL = [(m, n) for m, n in ALL if n not in gc.BIG]
LARGE = [(m, n) for m, n in ALL if n in gc.BIG]


def _claims(mode, family=None, **kw):
    out = []
    for n in gc.NAMES:
        c = gc.realise(n, mode)
        if (family is None or c['family'] == family) and all(c.get(k) == v for k, v in kw.items()):
            out.append((c, c['claims']))
    return out


# ------------------------------------------------------------------------------------------ the plan, against the launcher by hand
def test_plan_replays_the_launcher_on_known_shapes():
    h, f = torch.bfloat16, torch.float32
    nat = lambda M, N, K: {'a': (0, K), 'b': (0, K), 'c': (0, N)}
    # tests/test_gpu_ops.py test_linear_fwd_bwd: (1000, 64, 2560) is its one split -- 16 tiles want 32 slices, 40 stages allow 10
    p = gc.plan('bf16', 'fwd', 1000, 64, 2560, h, h, h, nat(1000, 64, 2560))
    assert (p['tile'], p['ksplit'], p['per'], p['reduce'], p['fast'], p['persist']) == (64, 10, 4, 'vec4', True, False)
    p = gc.plan('bf16', 'fwd', 1000, 64, 2560, f, f, f, nat(1000, 64, 2560))
    assert (p['ksplit'], p['depth'], p['passes']) == (10, 1, 0)
    # 256 tiles of 128: the big tile without a split, persistent, one round
    p = gc.plan('bf16', 'fwd', 2048, 2048, 512, h, h, h, nat(2048, 2048, 512))
    assert (p['tile'], p['ksplit'], p['persist'], p['rounds'], p['depth'], p['passes']) == (128, 1, True, 1, 2, 1)
    # 189 tiles of 128 do not reach 192 workgroups without a split and K = 384 never splits: 64-wide, 750 tiles, one round
    p = gc.plan('bf16', 'fwd', 7968, 384, 384, h, h, h, nat(7968, 384, 384))
    assert (p['tile'], p['ntiles'], p['grid'], p['rounds']) == (64, 750, 750, 1)
    # fp32: BK = 16, f32 tiles leave in 2 (64-wide) or 4 (128-wide) row slabs
    assert gc.plan('fp32', 'fwd', 72, 80, 20, f, f, f, nat(72, 80, 20), force_tile=64)['passes'] == 2
    assert gc.plan('fp32', 'fwd', 72, 80, 20, f, f, f, nat(72, 80, 20), force_tile=128)['passes'] == 4
    assert gc.plan('bf16', 'fwd', 72, 80, 72, h, h, f, nat(72, 80, 72), force_tile=128)['passes'] == 2
    # a 16-bit C += is never FAST without a split; with one, C is the reduce kernel's
    assert not gc.plan('bf16', 'fwd', 72, 80, 72, h, h, h, nat(72, 80, 72), accumulate=1)['fast']
    assert gc.plan('bf16', 'fwd', 72, 80, 512, h, h, h, nat(72, 80, 512), accumulate=1, force_ksplit=4)['fast']
    # every slice owns a stage: 5 stages / 4 asked -> 3 slices of 2, 2, 1;  17 / 16 -> 9
    assert gc.plan('bf16', 'fwd', 72, 80, 5 * 64, h, h, h, nat(72, 80, 320), force_ksplit=4)['ksplit'] == 3
    assert gc.plan('bf16', 'fwd', 72, 80, 17 * 64, h, h, h, nat(72, 80, 1088), force_ksplit=16)['ksplit'] == 9


def test_the_families_are_present():
    fam = {f: [n for n in gc.NAMES if gc.SPECS[n]['family'] == f] for f in gc.FAMILIES}
    assert sum(len(v) for v in fam.values()) == len(gc.NAMES) and all(fam.values())
    assert len(set(gc.NAMES)) == len(gc.NAMES)
    for mode in gc.MODES:
        assert set(gc.names_for(mode)) <= set(gc.NAMES)
    assert gc.names_for('bf16') == gc.names_for('fp16') and len(gc.names_for('fp32')) < len(gc.names_for('bf16'))
    for mode in gc.MODES:                                      # a case is dropped only where an earlier one is the same launch
        keys = {gc.realise(n, mode)['key'] for n in gc.names_for(mode)}
        assert keys == {gc.realise(n, mode)['key'] for n in gc.NAMES} and len(keys) == len(gc.names_for(mode))


@pytest.mark.parametrize('mode', gc.MODES)
def test_kloop_family(mode):
    g = gc.CFG[mode]
    for entry in gc.ENTRIES:
        for tile in (64, 128):
            got = {}
            for c, cl in _claims(mode, 'kloop', entry=entry, tile=tile):
                assert cl['tile'] == tile and cl['ksplit'] == 1
                if cl['fast']:
                    got.setdefault(cl['depth'], set()).add((cl['nk'], c['K'] - (cl['nk'] - 1) * g['BK']))
                else:
                    assert cl['depth'] == 1
            depths = {1, 2} if mode != 'fp32' else ({2} if entry == 'fwd' else {1})     # fp32: KC raw ring only, no raw transposer
            assert set(got) == depths, (entry, tile, got)
            for d in depths:                                   # the while (>= 4) body zero and one times, the three peeled drains
                assert got[d] == {(s, t) for s in range(1, 6) for t in (g['CE'], g['BK'])}
            gen = [c for c, cl in _claims(mode, 'kloop', entry=entry, tile=tile) if not cl['fast']]
            assert {c['K'] for c in gen if c['K'] % g['CE']} == {3, g['BK'] + 3, 2 * g['BK'] + 3}
            if entry != 'fwd':
                assert any(c['M'] % g['PM'] and c['N'] % g['PM'] and c['K'] % g['CE'] == 0 for c in gen)


@pytest.mark.parametrize('mode', gc.MODES)
def test_edges_family(mode):
    vals = {1, 15, 17, 63, 65, 127, 129}
    for tile in (64, 128):
        for entry in gc.ENTRIES:
            cs = _claims(mode, 'edges', entry=entry, tile=tile)
            assert vals <= {c['M'] for c, _ in cs} and vals <= {c['N'] for c, _ in cs}
        cs = _claims(mode, 'edges', entry='fwd', tile=tile)
        assert all(cl['tile'] == tile and cl['ksplit'] == 1 for _, cl in cs)
        for ot in {c['ot'] for c, _ in cs}:
            epc = 16 // gc.esize(ot)
            tail = [c for c, cl in cs if cl['fast'] and c['ot'] == ot and c['N'] % epc and c['lay']['c'][1] % epc == 0]
            assert any(c['N'] == 131 and c['lay']['c'][1] == 136 and not c['acc'] for c in tail)                  # store_tail
            assert any(c['N'] % 4 for c in tail)
            if ot == torch.float32:                            # store_tail_acc, with and without the ReLU
                assert {c['relu'] for c in tail if c['acc'] and c['N'] == 131} == {0, 1}
        slabs = [(c, cl) for c, cl in cs if c['M'] == 128 and c['ot'] == torch.float32 and cl['fast']]
        want = {('fp32', 64): 2, ('fp32', 128): 4}.get((mode, tile), 2 if tile == 128 else 1)
        assert slabs and all(cl['passes'] == want for _, cl in slabs) and {c['acc'] for c, _ in slabs} == {0, 1}
        assert any(not cl['fast'] and c['N'] % 4 for c, cl in cs)


@pytest.mark.parametrize('mode', gc.MODES)
def test_epilogue_family(mode):
    for tile in (64, 128):
        for fast in (True, False):
            seen = {(c['bias'], c['relu'], c['acc'], c['ot']) for c, cl in _claims(mode, 'epilogue', entry='fwd', tile=tile)
                    if cl['fast'] == fast and cl['ksplit'] == 1}
            ots = {torch.float32} | ({gc.h16_of(mode)} if mode != 'fp32' else set())
            want = {(b, r, a, ot) for b in (0, 1) for r in (0, 1) for a in (0, 1) for ot in ots}
            if fast:
                want = {w for w in want if not (w[2] and gc.esize(w[3]) == 2)}     # a 16-bit += is the generic kernel's
            assert seen == want, (tile, fast)
    for entry in ('dgrad', 'wgrad'):
        assert {c['acc'] for c, _ in _claims(mode, 'epilogue', entry=entry)} == {0, 1}


def test_types_family():
    for mode in ('bf16', 'fp16'):
        h, f = gc.h16_of(mode), torch.float32
        for entry in gc.ENTRIES:                               # the case labels of gemm_dispatch_bf16, all on the FAST kernel
            seen = {(c['at'], c['bt'], c['ot']) for c, cl in _claims(mode, 'types', entry=entry) if cl['fast']}
            assert seen == {(a, b, o) for a in (h, f) for b in (h, f) for o in ((h, f) if entry != 'wgrad' else (f,))}
    assert all(c['at'] == c['bt'] == c['ot'] == torch.float32 for c, _ in _claims('fp32'))


@pytest.mark.parametrize('mode', gc.MODES)
def test_layout_family(mode):
    for entry in gc.ENTRIES:
        cs = {c['name'].split(entry + '_', 1)[1]: cl for c, cl in _claims(mode, 'layout', entry=entry)}
        for tag in ('aoff1', 'boff1', 'coff1', 'lda1', 'ldb1', 'ldc1'):
            assert not cs[tag]['fast'] and cs[tag]['depth'] == 1, (entry, tag)
        for tag in ('lda_chunk', 'ldb_chunk', 'ldc_chunk'):
            assert cs[tag]['fast'], (entry, tag)
    c = gc.realise('layout_fwd_ldc1', mode)
    assert c['lay']['c'][1] % 2 == 1


@pytest.mark.parametrize('mode', gc.MODES)
def test_splitk_family(mode):
    cs = _claims(mode, 'splitk')
    forced = [(c, cl) for c, cl in cs if c['ksplit']]
    assert {(cl['nk'], c['ksplit'], cl['ksplit']) for c, cl in forced} == {(5, 4, 3), (8, 8, 8), (17, 16, 9), (12, 12, 12), (17, 17, 17)}
    assert all(cl['fast'] and cl['passes'] == 0 for _, cl in forced)          # a split launch is FAST whatever C is: the reduce writes it
    for nk, ks in ((5, 3), (8, 8), (17, 9), (12, 12), (17, 17)):
        sub = [(c, cl) for c, cl in forced if (cl['nk'], cl['ksplit']) == (nk, ks) and c['entry'] == 'fwd' and cl['tile'] == 64]
        assert {cl['reduce'] for _, cl in sub} == {'vec4', 'scalar'}
        assert any(c['N'] % 4 for c, _ in sub) and any(c['N'] % 4 == 0 and c['lay']['c'][1] % 2 for c, _ in sub)
        for red in ('vec4', 'scalar'):
            eps = {(c['bias'], c['relu'], c['acc'], gc.esize(c['ot'])) for c, cl in sub if cl['reduce'] == red}
            assert {(0, 0, 0, 4), (1, 1, 1, gc.esize(gc.dtype_of('h', mode)))} <= eps
        # 3 x 2 tiles (3 x 3 at N = 131): the swizzle moves something, and the two tile sizes leave different stamp counts
        assert all(cl['ntiles'] == (9 if c['N'] == 131 else 6) and cl['t128'] != cl['t64'] for c, cl in sub)
    assert {cl['per'] for c, cl in forced if (cl['nk'], cl['ksplit']) == (5, 3)} == {2}
    assert any(cl['tile'] == 128 and cl['ksplit'] >= 8 and cl['ntiles'] == 6 for _, cl in forced)
    assert {c['entry'] for c, cl in forced if cl['ksplit'] >= 8} == set(gc.ENTRIES)
    (c, cl), = [(c, cl) for c, cl in cs if not c['ksplit']]
    assert (c['M'], c['N'], c['K'], c['tile']) == (97, 64, 2560, 0) and cl['ksplit'] > 1 and cl['tile'] == 64


@pytest.mark.parametrize('mode', gc.MODES)
def test_tilemap_and_persist_families(mode):
    for tile in (64, 128):
        cs = _claims(mode, 'tilemap', tile=tile)
        assert all((c['M'] + tile - 1) // tile == 9 and (c['N'] + tile - 1) // tile == 3 and cl['tile'] == tile for c, cl in cs)
        assert {c['entry'] for c, cl in cs if not cl['persist'] and cl['fast']} == {'dgrad', 'wgrad'}
        assert any(c['entry'] == 'fwd' and not cl['fast'] for c, cl in cs)
        assert any(cl['persist'] and cl['rounds'] == 1 for _, cl in cs)
    cs = _claims(mode, 'persist')
    assert all(cl['persist'] and cl['rounds'] == 2 and cl['ksplit'] == 1 and cl['nk'] == 3 for _, cl in cs)
    assert {(cl['tile'], cl['ntiles'], cl['grid'], c['tile']) for c, cl in cs} == {(64, 1056, 1024, 64), (128, 529, 512, 0)}
    assert {cl['depth'] for _, cl in cs} == ({1, 2} if mode != 'fp32' else {2})
    assert all((c['M'] + 63) // 64 % 8 == 1 for c, cl in cs if cl['tile'] == 64)


@pytest.mark.parametrize('mode', gc.MODES)
def test_grouped_family(mode):
    gp = gc.grouped_plan(mode)
    cs = {c['name']: c for c, _ in _claims(mode, 'grouped')}
    assert set(gp) == set(cs) and all(c['acc'] and c['ot'] == torch.float32 for c in cs.values())
    big = [n for n, v in gp.items() if v == 128]
    assert len([n for n in big if n.startswith('grouped_512x512')]) == 8 and 'grouped_200x136_ragged' in big
    assert sum(((cs[n]['M'] + 127) // 128) * ((cs[n]['N'] + 127) // 128) for n in big) >= 128
    assert any(cs[n]['M'] % 128 and cs[n]['N'] % 128 for n in big)                       # ragged last tiles on the big tile
    assert gp['grouped_72x52_off1'] == 'standalone' and gp['grouped_72x52'] == 64 and gp['grouped_20x12'] == 64
    if mode != 'fp32':                                         # (fp32 has one type pair: the lone item joins the 512s)
        c = cs['grouped_136x100_lone']
        assert gp[c['name']] == 64 and c['M'] >= 128 and c['N'] >= 96                    # big by shape, alone in its type pair
        assert {(gc.esize(c['at']), gc.esize(c['bt'])) for n, c in cs.items() if gp[n] != 'standalone'} == {(2, 2), (4, 2), (2, 4), (4, 4)}
    assert any(c['M'] % 64 and c['N'] % 64 for n, c in cs.items() if gp[n] == 64)


def test_the_claims_reach_every_path():
    cl = [c for mode in gc.MODES for _, c in _claims(mode)]
    for key, vals in (('tile', {64, 128}), ('fast', {True, False}), ('persist', {True, False}), ('depth', {1, 2}),
                      ('passes', {0, 1, 2, 4}), ('reduce', {'none', 'vec4', 'scalar'}), ('swizzle', {True, False})):
        assert {c[key] for c in cl} == vals, key
    assert {c['tile'] for c in cl if c['rounds'] > 1} == {64, 128}
    assert max(c['ksplit'] for c in cl) >= 16                  # the reduce's 8-slab loop twice
    for mode in ('bf16', 'fp16'):                              # 16-bit compute alone reaches both depths, 1 and 2 passes and both tiles
        m = [c for _, c in _claims(mode)]
        assert {(c['tile'], c['depth']) for c in m if c['fast']} == {(t, d) for t in (64, 128) for d in (1, 2)}
        assert {c['passes'] for c in m} == {0, 1, 2}
    assert {c['passes'] for _, c in _claims('fp32')} == {0, 2, 4}


# ------------------------------------------------------------------------------------------ the bound holds the floor and has teeth
def _floor_and_mutants(mode, name):
    c = gc.realise(name, mode)
    ops = gc.operands(c)
    refs = gc.reference(c, ops)
    ref, S, _ = refs
    got = gc.floor(c, ops)
    bad = gc.violations(c, got, ref, S)
    assert not bool(bad.any()), gc.worst(c, got, ref, S)
    ratio = ((got.double() - ref).abs() / gc.bound(c, ref, S).clamp_min(1e-300)).max()
    assert float(ratio) <= 0.75, float(ratio)                  # room for another summation order
    applicable = 0
    for kind in gc.MUTANTS:
        m = gc.mutant(c, kind, ops, refs)
        if m is None:
            assert (kind == 'slab' and c['claims']['ksplit'] == 1) or (kind == 'bias_tail' and not c['bias']) or \
                   (kind == 'frag_swap' and c['N'] < 8), kind
            continue
        out, region = m
        applicable += 1
        v = gc.violations(c, out.to(c['ot']), ref, S)
        assert bool(region.any()) and bool(v[region].any()), (kind, 'not caught')
        assert not bool(v[~region].any()), (kind, 'reaches outside its region')
    assert applicable >= 2


@pytest.mark.parametrize('mode,name', SMALL)
def test_floor_within_bound_and_mutants_caught(mode, name):
    _floor_and_mutants(mode, name)


@pytest.mark.parametrize('mode,name', LARGE)
def test_floor_within_bound_and_mutants_caught_large(mode, name):
    _floor_and_mutants(mode, name)
