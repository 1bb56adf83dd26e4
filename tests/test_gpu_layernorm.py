"""GPU (-m gpu): the LayerNorm kernels (csrc/norm.hip) through otr_add_layernorm_fwd / _bwd / _bwd_skip, otr_add_layernorm2_* and
otr_add_layernorm3_*, per output element, in both libraries (16-bit type bf16 and fp16).

Every case of tests/layernorm_cases.py (checked on the CPU by tests/test_layernorm_cases.py) runs with every operand and output inside a
larger buffer whose guard rows before and after hold NaN; outputs are pre-filled with NaN, `partial` too, dgamma / dbeta / da_colsum
with known non-zero values.  After the call
  - every output element is within its bound of the float64 reference (layernorm_cases.reference; no norm anywhere) and none is NaN,
  - a 16-bit twin beside an fp32 output is its RNE rounding bit for bit,
  - guard rows, inputs and outputs the call was not asked for keep their bits,
  - with `partial`: every one of the 3 / 5 / 7 d columns of every row is finite, the column sums meet the bounds, dgamma / dbeta /
    da_colsum are untouched, and a second run gives the same bits; with da = NULL segment 2 of `partial` keeps what it held (the header
    says so); without `partial` dgamma / dbeta / da_colsum hold the old value plus the gradient,
  - da of a masked row and of a dropped element is exactly 0, and the forward's dropped set is exactly the numpy mask.
Two autograd-level tests use the same reference: ops.residual_layernorm(lp_only=True) (the 16-bit output, the 16-bit dy coming back) and
ops.add_layernorm with a_bias on the atomics path and on the deferred (partial sums, grouped column sums) path.
A failure names the case, output, row, column and float4 slot.  Every test adds its worst error / bound ratio per library, entry and
family to parity_out/layernorm_parity.json (or under $OTR_PARITY_DIR) before it asserts: `worst` over the outputs that exist in fp32,
`worst16` over those that exist in the 16-bit type only (y16 of lp_only, a 16-bit da), whose rounding takes its share of the bound
whole.

The bounds were derived (the docstring of tests/layernorm_cases.py), not fitted to these figures.  Measured on MI355X, worst error /
bound over every case of a library and entry:
  library  fwd    fwd2   fwd3   bwd    bwd2   bwd3   16-bit-only outputs
  bf16     0.50   0.51   0.70   0.48   0.46   0.42   1.00
  fp16     0.50   0.51   0.70   0.48   0.46   0.42   1.00
(the fp32 outputs do not depend on the library's 16-bit type where `a` is fp32, and the 16-bit `a` of a case holds other values in the
other type without moving the worst element).  By family: unit 0.50, offset 0.26, const 0.49, outlier 0.50, tiny 0.70, masked 0.49.
0.50 is z (one rounding of u |z| against u (|x| + 2 |s a| + |z|)) and the backward's dx = dz + skip on outlier rows (one rounding
against 2 u); 0.70 is rstd on the tiny rows, where var + eps and the rsqrt are all there is: 1.5 u of the 2 u allowed.  The outputs
that exist in the 16-bit type only reach 0.98 .. 1.00 of a bound that is their rounding and little else.
Three mutations of csrc/norm.hip were run against this module (wrong values only, every load and store in bounds), each fails it:
the rows past M of the last backward workgroup counted in dgamma / dbeta (134 tests: every single-LayerNorm backward with M % 8 != 0,
the autograd-level tests among them); beta1 where beta2 belongs in the third LayerNorm's recomputation (90: every bwd3 case); the
clamped loads of a partly filled last float4 slot counted in the row sums (246: every backward case with such a slot, by dx, dgamma
and dbeta, and no other).
The masked-row cases (family `masked`: NaN and Inf in the masked rows of `a`) fail on the kernel as it was before the row mask became a
select -- z, y, mean and rstd of every masked row are NaN there -- and pass on this one."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import layernorm_cases as lc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
CASES = [(m, n) for m in lc.MODES for n in lc.NAMES]
SEGMENTS = ('dgamma', 'dbeta', 'dacol', 'dgamma2', 'dbeta2', 'dgamma3', 'dbeta3')
ONLY16 = ('y16', 'y316', 'da')
PREFILL = 0.5
REPORT = {}


def _report(c, rat):
    key = '%s/%s/%s' % (c['mode'], c['entry'], c['family'])
    rec = REPORT.setdefault(key, {'cases': 0, 'worst': 0.0, 'at': '', 'worst16': 0.0})
    rec['cases'] += 1
    for k, q in rat.items():
        only16 = (k in ('y16', 'y316') and c['lp_only']) or (k == 'da' and c['at'] == 'h')
        if k in ('y16', 'y316') and not only16:
            continue                                           # a twin: judged bit for bit against the fp32 output
        v = float(q.max()) if q.size else 0.0
        f = 'worst16' if only16 else 'worst'
        if not v <= rec[f]:
            rec[f] = float('%.3g' % v)
            if not only16:
                rec['at'] = '%s:%s' % (c['name'], k)
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'layernorm_parity.json'), 'w') as f:
        json.dump(REPORT, f, sort_keys=True, indent=None, separators=(',', ':'))


def _lib(mode):
    from opentransformer_amd import ops, _lib as L
    ops.set_compute_dtype(mode)
    return L.load(), L


@pytest.fixture(autouse=True)
def _back_to_bf16():
    from opentransformer_amd import ops
    try:
        yield
    finally:
        ops.defer_weight_grads(False)
        ops.discard_pending_weight_grads()
        ops.set_compute_dtype('bf16')


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """a tensor of `shape` inside a larger buffer: guard rows (GUARD_ROWS of the last dimension, at least 16 elements) of NaN before and
    after it; `value` (array or number) fills the tensor itself, NaN where none is given"""

    def __init__(self, shape, dtype=torch.float32, value=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.lead = (max(lc.GUARD_ROWS * shape[-1], 16) + 15) // 16 * 16
        host = torch.full((self.lead + self.n + self.lead,), NAN, dtype=dtype)
        if value is not None:
            v = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32)) if isinstance(value, np.ndarray) else torch.tensor(float(value))
            host[self.lead:self.lead + self.n] = v.reshape(-1).to(dtype) if v.dim() else v.to(dtype)
        self.buf = host.to(DEV)
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.lead * self.buf.element_size())

    def view(self):
        return self.buf[self.lead:self.lead + self.n].view(self.shape)

    def numpy(self):
        return self.view().float().cpu().numpy()

    def bits(self):
        return self.view().view(BITS[self.buf.dtype])

    def guards_kept(self):
        b, lo, hi = BITS[self.buf.dtype], self.lead, self.lead + self.n
        return torch.equal(self.buf.view(b)[:lo], self.before.view(b)[:lo]) and torch.equal(self.buf.view(b)[hi:], self.before.view(b)[hi:])

    def untouched(self):
        b = BITS[self.buf.dtype]
        return torch.equal(self.buf.view(b), self.before.view(b))


def _p(b):
    return b.ptr() if b is not None else None


def _launch(lib, L, c, o):
    """one call of the case's entry on fresh guarded buffers: (inputs, outputs) as {name: Buf}"""
    M, d, e = c['M'], c['d'], c['entry']
    h, hcode = lc.h16_of(c['mode']), lib.otr_half_type()
    at = h if c['at'] == 'h' else torch.float32
    I, O = {}, {}

    def inp(k, dtype=torch.float32, key=None):
        v = o[key or k]
        I[k] = Buf(v.shape, dtype, v) if v is not None else None
        return _p(I[k])

    def out(k, shape, dtype=torch.float32, value=None, wanted=True):
        if not wanted:
            return None
        O[k] = Buf(shape, dtype, value)
        return _p(O[k])

    mask = torch.from_numpy(o['amask']).to(DEV) if o['amask'] is not None else None
    seed = torch.from_numpy(np.array([lc.SEED], dtype=np.uint64).view(np.int64)).to(DEV)
    sp = C.c_void_p(seed.data_ptr()) if c['p'] else None
    desc = L.LnDesc(M, d, hcode if (c['at'] == 'h' and c['has_a']) else L.OTR_F32, lc.EPS, c['p'], c['rng_offset'], c['a_scale'],
                    mask.data_ptr() if mask is not None else None, hcode if c['dy16'] else L.OTR_F32)
    keepalive = (mask, seed)
    gb = lambda *ks: [inp(k) for k in ks]
    if e[0] == 'f':
        x, a = inp('x'), (inp('a', at) if c['has_a'] else None)
        st = lambda *ks: [out(k, (M,)) for k in ks]
        if e == 'fwd':
            y = out('y', (M, d), wanted=not c['lp_only'])
            rc = lib.otr_add_layernorm_fwd(C.byref(desc), x, a, *gb('gamma1', 'beta1'), sp, y, out('y16', (M, d), h),
                                           out('z', (M, d), wanted=c['z_out']), *st('mean', 'rstd'), _stream())
        elif e == 'fwd2':
            rc = lib.otr_add_layernorm2_fwd(C.byref(desc), x, a, *gb('gamma1', 'beta1', 'gamma2', 'beta2'), sp, out('y', (M, d)),
                                            out('y16', (M, d), h), out('z', (M, d)), *st('mean', 'rstd', 'mean2', 'rstd2'), _stream())
        else:
            rc = lib.otr_add_layernorm3_fwd(C.byref(desc), x, a, *gb('gamma1', 'beta1', 'gamma2', 'beta2', 'gamma3', 'beta3'), sp,
                                            out('y', (M, d)), out('y3', (M, d), wanted=not c['lp_only']), out('y316', (M, d), h),
                                            out('z', (M, d)), *st('mean', 'rstd', 'mean2', 'rstd2', 'mean3', 'rstd3'), _stream())
    else:
        nseg = {'bwd': 3, 'bwd2': 5, 'bwd3': 7}[e]
        dy = inp('dy', h if c['dy16'] else torch.float32)
        z, mean, rstd = inp('z'), inp('mean'), inp('rstd')
        if c['skip'] == 'alias':                               # dx starts as the skip gradient and is read and written in place
            dx = skip = out('dx', (M, d), value=o['skip'])
        else:
            skip, dx = inp('skip'), out('dx', (M, d))
        da = out('da', (M, d), at, wanted=c['has_a'])
        part = out('partial', (c['nblk'], nseg * d), wanted=c['partial'])
        assert c['nblk'] == lib.otr_add_layernorm_bwd_partial_rows(M)
        if e == 'bwd':
            sums = [out(k, (d,), value=lc.prior(d, i)) for i, k in enumerate(SEGMENTS[:3])]
            if c['skip'] == 'none':
                rc = lib.otr_add_layernorm_bwd(C.byref(desc), dy, z, mean, rstd, inp('gamma1'), sp, dx, da, *sums, part, _stream())
            else:
                rc = lib.otr_add_layernorm_bwd_skip(C.byref(desc), dy, z, mean, rstd, inp('gamma1'), sp, skip, dx, da, *sums, part, _stream())
        elif e == 'bwd2':
            rc = lib.otr_add_layernorm2_bwd(C.byref(desc), dy, z, mean, rstd, *gb('gamma1', 'beta1'), inp('mean2'), inp('rstd2'), inp('gamma2'),
                                            sp, skip, dx, da, part, _stream())
        else:
            rc = lib.otr_add_layernorm3_bwd(C.byref(desc), dy, inp('dy3', h if c['dy3_16'] else torch.float32),
                                            hcode if c['dy3_16'] else L.OTR_F32, z, mean, rstd, *gb('gamma1', 'beta1'), inp('mean2'), inp('rstd2'),
                                            *gb('gamma2', 'beta2'), inp('mean3'), inp('rstd3'), inp('gamma3'), sp, skip, dx, da, part, _stream())
    torch.cuda.synchronize()
    del keepalive
    assert rc == 0, (c['name'], rc, lib.otr_last_error_string())
    return I, O


def _collect(c, O):
    """the outputs as arrays under the reference's names; the column sums of `partial` in float64"""
    d = c['d']
    got = {k: b.numpy() for k, b in O.items() if k != 'partial'}
    if c['entry'][0] == 'b' and c['partial']:
        part = O['partial'].view().double().cpu().numpy()
        for i in range(part.shape[1] // d):
            if i == 2 and not c['has_a']:
                continue
            got[SEGMENTS[i]] = part[:, i * d:(i + 1) * d].sum(0)
    elif c['entry'] == 'bwd' and not c['has_a']:
        got.pop('dacol')
    return got


def _judge(c, got, ref=None):
    rat = lc.ratios(c, got, ref)
    _report(c, rat)
    w = lc.worst(c, rat)
    assert w[0] <= 1.0, '%s: %s is outside its bound: error / bound %.3g at row %d, column %d (float4 slot %d)' % (
        c['name'], w[1], w[0], w[2], w[3], w[4])
    return rat


def _twin(c, O, y, y16):
    if y in O and y16 in O:
        h = lc.h16_of(c['mode'])
        same = O[y].view().to(h).view(torch.int16) == O[y16].bits()
        assert bool(same.all()), '%s: %s is not the RNE rounding of %s at %r' % (c['name'], y16, y, (~same).nonzero()[0].tolist())


@pytest.mark.parametrize('mode,name', CASES, ids=['%s-%s' % p for p in CASES])
def test_layernorm_case(mode, name):
    lib, L = _lib(mode)
    c = lc.realise(name, mode)
    o = lc.operands(c)
    M, d = c['M'], c['d']
    I, O = _launch(lib, L, c, o)
    got = _collect(c, O)
    _judge(c, got)
    for k, b in I.items():
        assert b is None or b.untouched(), '%s: the input %s was written' % (name, k)
    for k, b in O.items():
        assert b.guards_kept(), '%s: the guard rows of %s were written' % (name, k)
    rowm = (o['amask'] != 0)[:, None] if o['amask'] is not None else np.ones((M, 1), dtype=bool)
    live = lc.keep_mask(c) & rowm                              # the elements of the branch that take part
    if c['entry'][0] == 'f':
        _twin(c, O, 'y', 'y16')
        _twin(c, O, 'y3', 'y316')
        if c['has_a'] and c['z_out']:
            moved = got['z'] != o['x']                         # bit-equal to x exactly where the branch was dropped or masked
            assert not moved[~live].any(), '%s: z differs from x at a dropped or masked element %r' % (name, np.argwhere(moved & ~live)[0])
            with np.errstate(invalid='ignore'):
                sa = np.abs(np.where(live, o['a'], 0).astype(np.float64) * float(lc.branch_scale(c)))
            must = live & (sa > 4 * lc.U * (np.abs(o['x']) + sa))
            assert moved[must].all(), '%s: a kept element of the branch did not reach z at %r' % (name, np.argwhere(must & ~moved)[0])
        return
    if c['has_a']:
        assert not (got['da'][~np.broadcast_to(live, (M, d))] != 0).any(), '%s: da of a masked row or dropped element is not 0' % name
    if not c['partial']:
        if not c['has_a']:
            assert O['dacol'].untouched(), '%s: da_colsum written without da' % name
        return
    part = O['partial'].view()
    seg2 = slice(2 * d, 3 * d)
    if c['has_a']:
        assert bool(torch.isfinite(part).all()), '%s: partial has unwritten or non-finite columns' % name
    else:                                                      # no da: segment 2 keeps what it held, the rest is written
        keep = torch.ones(part.shape[1], dtype=torch.bool, device=DEV)
        keep[seg2] = False
        assert bool(torch.isfinite(part[:, keep]).all()), '%s: partial has unwritten or non-finite columns' % name
        assert bool(torch.isnan(part[:, seg2]).all()), '%s: segment 2 of partial was written without da' % name
    for k in SEGMENTS[:3]:
        assert k not in O or O[k].untouched(), '%s: %s written although partial was given' % (name, k)
    _, O2 = _launch(lib, L, c, o)                              # no atomics: the same bits again
    for k in O:
        assert torch.equal(O[k].bits(), O2[k].bits()), '%s: %s differs between two runs' % (name, k)


# ------------------------------------------------------------------------------------------ through autograd
def _np(t):
    return t.detach().float().cpu().numpy()


def _params(d, g, inplace):
    ps = []
    for k in range(3):
        v = (0.2 * torch.randn(d, generator=g) + (1.0 if k == 0 else 0.0)).to(DEV).requires_grad_(True)
        if inplace:
            v.grad = torch.full((d,), PREFILL, device=DEV)
            v._otr_grad_inplace = True
        ps.append(v)
    return ps


def _fwd_operands(x, a, gamma, beta):
    return dict(x=_np(x), a=_np(a), gamma1=_np(gamma), beta1=_np(beta), amask=None)


def _bwd_operands(fo, fref, z, dz_in, dy, skip):
    """the backward operands behind a forward the kernel ran itself: its statistics are within the forward bounds of the reference's"""
    (mu, bmu), (r, br) = fref['mean'], fref['rstd']
    return dict(fo, z=z, mean=mu, rstd=r, dmean=bmu, drstd=br, dz_in=dz_in, dy=dy, skip=skip)


@pytest.mark.parametrize('mode', lc.MODES)
def test_residual_layernorm_lp_only_through_autograd(mode):
    """ops.residual_layernorm(lp_only=True): z and the 16-bit y alone leave, d y comes back in the 16-bit type (otr_ln_desc_t.dy_dtype)
    together with the gradient of z as the skip operand"""
    from opentransformer_amd import ops
    ops.set_compute_dtype(mode)
    M, d, h = 9, 260, lc.h16_of(mode)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, d, generator=g).to(DEV).requires_grad_(True)
    a = torch.randn(M, d, generator=g).to(h).to(DEV).requires_grad_(True)
    gamma, beta, _ = _params(d, g, False)
    z, y16 = ops.residual_layernorm(x, a, 0.5, 0.0, gamma, beta, eps=lc.EPS, lp_only=True)
    assert y16.dtype == h and z.dtype == torch.float32
    gz, gy = torch.randn(M, d, generator=g).to(DEV), torch.randn(M, d, generator=g).to(h).to(DEV)
    dx, da, dg, db = torch.autograd.grad((z, y16), (x, a, gamma, beta), (gz, gy))
    torch.cuda.synchronize()
    assert da.dtype == h
    cf = lc.custom(mode, 'fwd', d, M, 'h', a_scale=0.5, lp_only=True, tag='autograd')
    fo = _fwd_operands(x, a, gamma, beta)
    got = {'z': _np(z), 'y16': _np(y16)}
    fref = lc.reference(cf, got, o=fo)
    _judge(cf, got, fref)
    cb = dict(lc.custom(mode, 'bwd', d, M, 'h', a_scale=0.5, dy16=True, skip='sep', tag='autograd'), old=0.0)
    bo = _bwd_operands(fo, fref, got['z'], np.zeros((M, d)), _np(gy), _np(gz))
    _judge(cb, {'dx': _np(dx), 'da': _np(da), 'dgamma': _np(dg), 'dbeta': _np(db)}, lc.reference(cb, o=bo))


@pytest.mark.parametrize('way', ['atomics', 'deferred'])
@pytest.mark.parametrize('mode', lc.MODES)
def test_add_layernorm_a_bias_through_autograd(mode, way):
    """ops.add_layernorm(a_bias=b): the bias gradient of the Linear behind the branch is the column sum of da, added into zero-filled
    rows by the kernel's atomics, or -- with in-place gradient buffers and deferral on -- left as per-workgroup partial sums that the
    grouped column sum at the end of the pass adds to what the buffers held"""
    from opentransformer_amd import ops
    ops.set_compute_dtype(mode)
    M, d, h = 17, 516, lc.h16_of(mode)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, d, generator=g).to(DEV).requires_grad_(True)
    a = torch.randn(M, d, generator=g).to(h).to(DEV).requires_grad_(True)
    gamma, beta, bias = _params(d, g, way == 'deferred')
    ops.defer_weight_grads(way == 'deferred')
    y = ops.add_layernorm(x, a, gamma, beta, 0.0, lc.EPS, a_bias=bias)
    gy = torch.randn(M, d, generator=g).to(DEV)
    y.backward(gy)
    torch.cuda.synchronize()
    assert ops._wq['w'] == [] and ops._wq['b'] == []
    cf = lc.custom(mode, 'fwd', d, M, 'h', z_out=False, tag='autograd')
    fo = _fwd_operands(x, a, gamma, beta)
    got = {'y': _np(y)}
    fref = lc.reference(cf, got, o=fo)
    _judge(cf, got, fref)
    twin = ops.lp_of(y)
    assert twin is not None and torch.equal(twin.view(torch.int16), y.detach().to(h).view(torch.int16))
    cb = dict(lc.custom(mode, 'bwd', d, M, 'h', tag='autograd_' + way), old=PREFILL if way == 'deferred' else 0.0)
    bo = _bwd_operands(fo, fref, fref['z'][0], fref['z'][1], _np(gy), None)
    assert a.grad.dtype == h
    _judge(cb, {'dx': _np(x.grad), 'da': _np(a.grad), 'dgamma': _np(gamma.grad), 'dbeta': _np(beta.grad), 'dacol': _np(bias.grad)},
           lc.reference(cb, o=bo))
