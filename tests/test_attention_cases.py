"""CPU: the attention cases of tests/attention_cases.py are what their names say, reference() is the dense formulation (torch.autograd
in float64, and the explicit gather of the oracle's relative-position attention), and floor() -- the emulated working precision --
stays inside the tolerances of tests/test_gpu_ops.py on every case, so that a failure on the GPU is the kernel's."""
import math

import pytest
import torch

from tests import attention_cases as ac


def _lens(c):
    return [int(x) for x in c['key_mask'].sum(1)]


# ------------------------------------------------------------------------------------------ the cases are what they say
def test_the_families_cover_the_grid():
    fam = {f: [n for n in ac.NAMES if ac.build(n)['family'] == f] for f in ac.FAMILIES}
    assert sum(len(v) for v in fam.values()) == len(ac.NAMES)
    sweep = {(ac.build(n)['dk'], n.rsplit('_', 1)[1]) for n in fam['sweep']}
    assert sweep == {(dk, fl) for dk in (16, 32, 64, 96, 128) for fl in ('aligned', 'off1', 'stride')}
    causal = {(ac.build(n)['Tq'], ac.build(n)['dk'], ac.build(n)['key_mask'] is not None) for n in fam['causal']}
    assert causal == {(T, dk, r) for T, dk in ((130, 64), (200, 64), (130, 32)) for r in (False, True)}
    mask = {(n.rsplit('_d', 1)[0], ac.build(n)['dk']) for n in fam['mask']}
    assert mask == {('mask_' + t, dk) for t in ('dead', 'first_block', 'alternating', 'middle_block') for dk in (64, 32)}
    cross = {(ac.build(n)['Tq'], ac.build(n)['Tk'], ac.build(n)['dk']) for n in fam['cross'] if n.startswith('cross_') and 'x' in n}
    assert cross == {(tq, tk, dk) for tq, tk in ((130, 70), (1, 1), (70, 1), (1, 200), (5, 49), (64, 65)) for dk in (64, 32)}
    assert {'cross_kv_slices', 'cross_wide_batch_stride'} <= set(fam['cross'])
    rel = {(ac.build(n)['Tq'], ac.build(n)['dk']) for n in fam['bias'] if ac.build(n)['rel_shift']}
    assert rel == {(T, dk) for T in (20, 32, 33, 70, 130) for dk in (16, 64, 96)}
    plain = [ac.build(n) for n in fam['bias'] if not ac.build(n)['rel_shift']]
    assert plain and all((c['Tq'], c['Tk']) == (70, 130) and tuple(c['bias'].shape) == (c['B'], c['H'], 70, 130) for c in plain)


@pytest.mark.parametrize('name', ac.NAMES)
def test_case_is_what_its_name_says(name):
    c = ac.build(name)
    B, H, Tq, Tk, dk, d = c['B'], c['H'], c['Tq'], c['Tk'], c['dk'], c['d']
    assert B <= 3 and H <= 3 and max(Tq, Tk) <= 200 and dk in (16, 32, 64, 96, 128)
    assert all(tuple(c[x].shape) == (B, T, d) for x, T in (('q', Tq), ('k', Tk), ('v', Tk), ('do', Tq)))
    assert c['key_mask'] is None or (tuple(c['key_mask'].shape) == (B, Tk) and c['key_mask'].dtype == torch.uint8)
    assert ac.dead_utterances(c) == c['claims']['dead']
    for mode in ac.MODES:
        assert ac.vec_ok(c, mode) == c['claims']['aligned'], mode
    assert ac.bias_vec4(c) == c['claims']['bias_vec4']
    adm = ac.admissible(c)
    dead_rows = ~adm.any(-1)[:, 0]                                                    # [B, Tq]
    assert [b for b in range(B) if bool(dead_rows[b].all())] == c['claims']['dead']
    assert not bool(dead_rows[[b for b in range(B) if b not in c['claims']['dead']]].any())     # no other row is without a key
    for x, T in (('q', Tq), ('k', Tk), ('v', Tk), ('o', Tq)):                        # the layout holds the operand without overlap
        off, bs, ts = c['lay'][x]
        assert ts >= d and bs >= T * ts - (ts - d) and off >= 0
        base, n, own = ac.owned(c['lay'][x], B, T, d)
        assert int(own.sum()) == B * T * d and n == base + (B - 1) * bs + (T - 1) * ts + d
    fam = c['family']
    if fam == 'sweep':
        assert (H * B) % 8 != 0                                                       # padding workgroups in the XCD-aware grid
        assert (Tq, Tk) == (70, 70) and (Tk + 63) // 64 == 2 and Tk - 64 == 6
        assert Tk in _lens(c) and 41 in _lens(c)
        if name.endswith('off1'):
            assert all((c['lay'][x][0] * es) % 16 != 0 and c['lay'][x][2] == d for x in 'qkvo' for es in (2, 4))
        if name.endswith('stride'):
            assert all(c['lay'][x][0] == 0 and c['lay'][x][2] % ce != 0 for x in 'qkvo' for ce in (4, 8))
    if fam == 'causal':
        assert c['causal'] and Tq == Tk and (Tq + 127) // 128 == 2 and (Tq + 63) // 64 >= 3
        assert Tq != 130 or Tq - 128 == 2
        if name.endswith('ragged'):
            assert min(_lens(c)) == 1 and max(_lens(c)) == Tk
    if fam == 'mask':
        km = c['key_mask']
        assert Tq == Tk == 130
        if 'dead' in name:
            assert _lens(c)[1] == 0 and _lens(c)[0] == Tk
        if 'first_block' in name:
            assert int(km[0, :64].sum()) == 0 and int(km[0, 64:].sum()) == Tk - 64
        if 'alternating' in name:
            assert km[0].tolist() == [1 - (j & 1) for j in range(Tk)] and km[1].tolist() == [j & 1 for j in range(Tk)]
        if 'middle_block' in name:
            assert int(km[0, 64:128].sum()) == 0 and int(km[0].sum()) == Tk - 64 and bool(km[0, 128:].all())
    if fam == 'cross':
        assert not c['causal'] and c['key_mask'] is not None and c['bias'] is None
        if name == 'cross_kv_slices':
            assert c['lay']['k'][2] == 6 * d and c['lay']['v'][2] == 6 * d and c['lay']['v'][0] - c['lay']['k'][0] == d
        if name == 'cross_wide_batch_stride':
            assert c['lay']['q'][1] > Tq * c['lay']['q'][2]
    if fam == 'bias':
        assert c['bias'] is not None and min(_lens(c)) < Tk and c['key_mask2'] is not None
        newly_masked = (c['key_mask'] != 0) & (c['key_mask2'] == 0)                      # what a second launch has to overwrite with zeros
        assert bool(newly_masked.any())
        if c['rel_shift']:
            P = 2 * Tq - 1
            assert c['ncol'] % 8 == 0 and P <= c['ncol'] < P + 8 and tuple(c['bias'].shape) == (B, Tq, H, c['ncol'])
            assert bool((c['bias'][..., P:] == ac.PAD_BIAS).all())
            assert c['claims']['bias_vec4'] == (Tq >= 33)
            band = ac.in_band(c)
            assert int(band.sum()) == Tq * Tk and not bool(band[:, P:].any())
            assert int(ac.bias_columns(c).min()) == 0 and int(ac.bias_columns(c).max()) == P - 1


# ------------------------------------------------------------------------------------------ reference() is the dense formulation
def _autograd(c, mode):
    """out, lse and the gradients of sum(out * do) by torch.autograd in float64 from masked_fill + softmax; the bias enters through
    torch.gather on a leaf in its own memory layout"""
    H, dk = c['H'], c['dk']
    x = ac.operands(c['name'], mode)
    q, k, v = (ac.heads(x[n].double(), H).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    do = ac.heads(x['do'].double(), H)
    s = q @ k.transpose(-1, -2)
    bias = None
    if c['bias'] is not None:
        bias = c['bias'].double().clone().requires_grad_(True)
        s = s + ac.dense_bias(dict(c, bias=bias))
    s = s * float(torch.tensor(1.0 / math.sqrt(dk), dtype=torch.float32))
    s = s.masked_fill(~ac.admissible(c), float('-inf'))
    out = torch.softmax(s, -1) @ v
    lse = torch.logsumexp(s, -1, keepdim=True)
    g = torch.autograd.grad(out, [q, k, v] + ([bias] if bias is not None else []), do)
    res = {'out': out.detach(), 'lse': lse.detach(), 'delta': (out.detach() * do).sum(-1, keepdim=True), 'dq': g[0], 'dk': g[1], 'dv': g[2]}
    if bias is not None:
        res['dbias'] = ac.bias_canonical(c, g[3])
    return res


@pytest.mark.parametrize('name', ac.NAMES)
def test_reference_is_autograd_of_the_dense_formulation(name):
    c = ac.build(name)
    mode = 'bf16' if c['dk'] % 32 else 'fp32'                                          # the formulas do not depend on the mode; both get used
    ref, want = ac.reference(name, mode), _autograd(c, mode)
    defined = [b for b in range(c['B']) if b not in c['claims']['dead']]               # softmax of a row without keys is NaN in torch
    for n, w in want.items():
        a = ref[n][defined]
        w = w[defined]
        assert bool(torch.isfinite(w).all()), n
        assert float((a - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), n
    for b in c['claims']['dead']:                                                     # the contract where torch has none
        assert bool((ref['lse'][b] == float('-inf')).all())
        assert all(float(ref[n][b].abs().max()) == 0.0 for n in ac.outputs(c) if n != 'lse')
    if c['key_mask'] is not None:                                                     # masked keys and pairs: exact zeros
        masked = c['key_mask'] == 0
        for b in range(c['B']):
            assert float(ref['dk'][b][:, masked[b]].abs().max() if bool(masked[b].any()) else 0.0) == 0.0
            assert float(ref['dv'][b][:, masked[b]].abs().max() if bool(masked[b].any()) else 0.0) == 0.0
    if c['bias'] is not None and c['rel_shift']:
        assert float(ref['dbias'][:, :, ~ac.in_band(c)].abs().max()) == 0.0


@pytest.mark.parametrize('T,h,dk', [(20, 2, 16), (33, 3, 16), (70, 2, 32)])
def test_reference_agrees_with_the_oracles_explicit_gather(T, h, dk):
    """oracle/otrans_oracle.py relpos_self_attention builds [B, h, T, 2T - 1] and gathers column j - i + T - 1; reference() reads the
    same un-shifted term through rel_shift.  The case is built from the oracle's own operands: (q + u), k, v and (q + v) p^T."""
    import torch.nn.functional as F
    from oracle import otrans_oracle as orc
    B, d = 2, h * dk
    g = torch.Generator().manual_seed(T)
    sd = {'qvk_proj.weight': torch.randn(3 * d, d, generator=g, dtype=torch.float64) / math.sqrt(d),
          'qvk_proj.bias': torch.randn(3 * d, generator=g, dtype=torch.float64) * 0.1,
          'pos_proj.weight': torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d),
          'posu': torch.randn(h, dk, generator=g, dtype=torch.float64) * 0.3, 'posv': torch.randn(h, dk, generator=g, dtype=torch.float64) * 0.3}
    x = torch.randn(B, T, d, generator=g, dtype=torch.float64)
    pos = orc.sinusoid(torch.arange(-(T - 1), T).reshape(1, -1), d).double()
    km = ac.prefix_mask([T, T - T // 4], T)
    ctx = orc.relpos_self_attention(sd, x, km.bool().unsqueeze(1), pos, h)
    q, k, v = torch.split(F.linear(x, sd['qvk_proj.weight'], sd['qvk_proj.bias']), d, dim=-1)
    q4 = q.reshape(B, T, h, dk)
    p = F.linear(pos, sd['pos_proj.weight']).reshape(2 * T - 1, h, dk)
    bd = torch.einsum('bthc,phc->bthp', q4 + sd['posv'], p)                            # [B, T, h, 2T - 1], un-shifted
    c = ac.make_case('oracle_relpos', B, h, T, T, dk, key_mask=km, bias='rel',
                     tensors={'q': (q4 + sd['posu']).reshape(B, T, d), 'k': k, 'v': v, 'bias': bd})
    out = ac.compute(c, 'fp32', False)['out'].permute(0, 2, 1, 3).reshape(B, T, d)
    # the case holds the operands as float32: 2^-24 relative on each, a few of them per score
    assert float((out - ctx).norm() / ctx.norm()) < 1e-6


# ------------------------------------------------------------------------------------------ floor() stays inside the tolerances
@pytest.mark.parametrize('name', ac.NAMES)
def test_floor_stays_within_the_tolerances(name):
    """every case is well conditioned: the emulated working precision meets the whole-tensor tolerances of tests/test_gpu_ops.py"""
    c = ac.build(name)
    for mode in ac.MODES:
        fd, tn = ac.floor_distances(name, mode), ac.tiny(name, mode)
        fl = ac.floor(name, mode)
        for n in ac.outputs(c):
            blocks, dist, norm = fd[n]
            assert bool(torch.isfinite(fl[n]).all() if n != 'lse' else not bool(torch.isnan(fl[n]).any())), (mode, n)
            assert ac.whole_ok(n, mode, dist, norm, tn[n], dist, 1.0), (mode, n, dist / max(norm, 1e-300), ac.tol_of(n, mode))
            assert tuple(blocks.shape) == tuple(tn[n].shape)


def test_a_wrong_tile_shows_in_its_block_and_not_in_the_whole():
    """what the blockwise measure is for: 16 rows of one head scaled by 1.1 pass the whole-tensor bf16 tolerance"""
    name, mode = 'sweep_d64_aligned', 'bf16'
    ref, fl = ac.reference(name, mode), ac.floor(name, mode)
    bad = fl['dk'].clone()
    bad[1, 2, 16:32] *= 1.1
    blocks, dist, norm = ac.distances(bad, ref['dk'])
    fblocks = ac.floor_distances(name, mode)['dk'][0]
    assert dist <= ac.tol_of('dk', mode) * norm
    assert float(blocks[1, 2, 1]) > 10 * float(fblocks[1, 2, 1]) + float(ac.tiny(name, mode)['dk'][1, 2, 1])
