"""Named cases for the LayerNorm kernels (csrc/norm.hip behind otr_add_layernorm_fwd / _bwd / _bwd_skip, otr_add_layernorm2_* and
otr_add_layernorm3_*), the float64 reference and the per-element bounds they are judged by.  No GPU here: tests/test_layernorm_cases.py
checks on the CPU that every case is what its name claims and that the bounds have teeth, tests/test_gpu_layernorm.py runs the cases
through the C ABI in both libraries (16-bit type bf16 / fp16).

A case name reads  <entry>_d<d>nv<NV><t|e>_M<M>q<M mod 4>o<M mod 8>_<a type>_<family>[_<options>]:  NV = ceil(d / 256) float4 slots per
lane, t = the last slot is partly filled (the backward clamps those loads to d - 4), q / o = rows in the last 4-row forward / 8-row
backward workgroup.  Families: unit N(0,1); offset (row means +-1e3, std 1); const (constant and all-zero rows among normal ones);
outlier (one 1e4 per row); tiny (x 1e-6); masked (a row mask, the masked rows of `a` hold NaN and Inf).

Reference, stage by stage in float64 from the exact fp32 / 16-bit input bits:
    z = x + s m drop a,  s = fp32(fp32(1 / (1 - p)) a_scale),  drop from the numpy restatement of otr_rand32 with the kernel's threshold
    arithmetic in float32, m the row mask applied as a FILL (a masked row contributes exactly 0, whatever `a` holds there);
    LN(v) = (v - mu) r gamma + beta,  mu = mean(v), r = (mean((v - mu)^2) + eps)^-1/2,  eps = float64(float32(eps)); LN1, LN2, LN3 chained.
    Backward of one LayerNorm with normalised input n and g = dy gamma:  d in = r (g - mean(g) - n mean(g n)),  dgamma = sum_rows dy n,
    dbeta = sum_rows dy; chained LN3 -> LN2 -> LN1, then dx = skip + dz, da = s m drop dx, da_colsum = sum_rows da.  The backward cases
    take z, mean and rstd (and mean2.. rstd3) as float64 values rounded to fp32, so they do not depend on the forward kernel, and the
    reference uses exactly those inputs, as the kernel does: n = (z - mean) rstd, y1 = n gamma + beta recomputed, and so on.

Bounds.  u = 2^-24, NV = ceil(d / 256), C = 4 NV + 10: the kernel's summation depth (4 serial adds per float4 slot, 6 butterfly steps)
plus 4 of slack.  Every quantity below is the float64 reference's; `din` is the bound on what the stage's input already carries (0 for a
stage that reads stored fp32 values); terms of second order in u are covered by the slack.
  z:        |z - ref| <= u (|x| + 2 |s a|) + u |z|            (one product, one sum -- or one fused multiply-add)
  forward of one LayerNorm, input v, t = v - mu:
    dmu   = C u mean|v| + mean(din)                            (a length-d fp32 sum in any order; the mean of the input's error)
    dt_j  = u (|v_j| + |mu|) + dmu + din_j                     (one subtraction of two numbers this large, from a mean off by dmu)
    dvar  = 2 mean(|t| dt) + mean(dt^2) + C u var              (d(t^2) = 2 |t| dt; the sum of squares again a length-d sum)
    rho   = dvar r^2 / 2 + 2 u                                 (d r / r = d var / (2 (var + eps)); the add of eps and the rsqrt round)
    |y_j - ref_j| <= dt_j r |gamma_j| + |t_j r gamma_j| (rho + 3 u) + u |beta_j| + eps_out |ref_j|
    |mean - mu| <= dmu + u |mu|,   |rstd - r| <= r rho
    y is judged from the kernel's OWN z where the call returns it (that is what the kernel holds in registers: din = 0); a chained
    stage takes the previous stage's y bound as its din.  eps_out = u for an fp32 output; a 16-bit twin beside an fp32 output must be
    its RNE rounding bit for bit; where the twin is the only output its unit roundoff (2^-8 bf16, 2^-11 fp16) times |ref| is added.
  backward (u here is u' = 2 u: every rounding is charged twice its unit roundoff.  The forward form has its slack in dt, |v_j| + |mu|
  against the |t_j| that is rounded; the backward terms have none, and a single rounding that dominates an element -- dx = dz + skip
  with a small dz -- comes as close to u as the data makes it.  The factor keeps such an element at half its bound.)
  backward of one LayerNorm, dy carrying ddy and the normalised input n carrying dn, g = dy gamma:
    dg_j  = |gamma_j| ddy_j + u |g_j|
    ds1   = mean(dg) + C u mean|g|                             s1 = mean(g)
    ds2   = mean(dg |n| + |g| dn) + (C + 2) u mean|g n|        s2 = mean(g n): two more roundings per term
    |out_j - ref_j| <= r (dg_j + ds1 + |n_j| ds2 + |s2| dn_j + 3 u (|g_j| + |s1| + |n_j s2|)) + 2 u |out_j|
    per row and column the dgamma term dy n is off by ddy |n| + |dy| dn + u |dy n|, the dbeta term dy by ddy.
    n = (z - mean) rstd from stored fp32 values: dn = 2 u |n|.  The recomputed y1 = n gamma + beta carries |gamma| dn + u |n gamma| + u |y1|,
    the next normalised input (y1 - mean2) rstd2 carries rstd2 (dy1 + u |y1 - mean2|) + u |.|, and y2 / LN3 the same again.
    d y2 + (LN3's input gradient) adds u |sum|; dx = dz + skip adds u |dx|; da = s drop dx one more rounding u |da|, and the unit
    roundoff of a 16-bit `a` type times |da|.
  column sums (dgamma, dbeta, da_colsum and their LN2 / LN3 twins) over M rows in nblk = ceil(M / 8) workgroups:
    sum_rows(term bounds) + (M + nblk + 4) u (|old| + sum_rows |term|)       (C enlarged by the rows and the atomics summed; plain u)
  a backward behind a forward the kernel ran itself (the autograd-level tests) reads statistics that are within the forward bounds of
  the reference's: dn grows by rstd (dz + dmean) + |z - mean| drstd.
None of this is fitted to what a GPU returns.

floor() is a plain fp32 emulation of the same arithmetic (numpy float32, one rounding per operation; z = x + s a as the one fused
multiply-add the compiler makes of `v += a * sc`) with the row sums in three orders: `lane`, the kernel's (four serial adds per float4
slot, slots one after another, a 64-lane butterfly); `pairwise` over the row; `serial`, the lane sums added one after another in place
of the butterfly.  A left-to-right sum of all d elements is not among them: its depth d - 1 is not the kernel's, and on the offset rows
at d = 1020 it uses the whole of dmu, as it should.  tests/test_layernorm_cases.py requires floor() to stay at or below 0.5 of the bound
on every case in every order.  The outputs that exist in the 16-bit type only are judged there before their rounding, against the fp32
part of their bound: |RNE(v) - v| <= unit roundoff |v| is exact arithmetic and is met with equality by some element of any large
tensor, so the rounded values are held to the whole bound (ratio <= 1) instead.
MUTANTS are the errors the bounds have to catch; each must exceed the bound on at least one named case:
  onepass     variance as mean(v^2) - mean^2                    last4       the last float4 of a row missing from the statistics
  padded      sums divided by NV 256 instead of d               noeps       eps left out
  no_s2       backward without the n mean(g n) term             phantom     the rows past M of the last 8-row workgroup in dgamma / dbeta
  beta1       LN3's recomputation of y2 with beta1 for beta2    colsum_pre  da column sums taken before a_scale / dropout
  drop_shift  dropout index shifted by one element              mask_mul    the row mask as a multiply (NaN / Inf in the masked rows)"""
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24
UB = 2 * U                                                 # what the backward bounds charge for one rounding
MODES = ('bf16', 'fp16')
UH = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
ENTRIES = ('fwd', 'bwd', 'fwd2', 'bwd2', 'fwd3', 'bwd3')
FAMILIES = ('unit', 'offset', 'const', 'outlier', 'tiny', 'masked')
ORDERS = ('lane', 'pairwise', 'serial')
MUTANTS = ('onepass', 'last4', 'padded', 'noeps', 'no_s2', 'phantom', 'beta1', 'colsum_pre', 'drop_shift', 'mask_mul')
# d -> (NV, lanes of the last float4 slot that hold data, 0 = all 64), M -> (M mod 4, M mod 8): written out, the test recomputes them
D_TABLE = {4: (1, 1), 8: (1, 2), 64: (1, 16), 252: (1, 63), 256: (1, 0), 260: (2, 1), 384: (2, 32), 512: (2, 0), 516: (3, 1), 768: (3, 0),
           772: (4, 1), 1020: (4, 63), 1024: (4, 0)}
M_TABLE = {1: (1, 1), 7: (3, 7), 8: (0, 0), 9: (1, 1), 17: (1, 1)}
EPS = 1e-5
SEED = 0x9E3779B97F4A7C15                                  # high word non-zero
RNG_OFFSET = 1000003
RNG_OFFSET_BIG = (1 << 32) + 12345                         # the index's high word takes part too
GUARD_ROWS = 2


def h16_of(mode):
    return torch.float16 if mode == 'fp16' else torch.bfloat16


def round_h16(v, mode):
    """float32 array rounded (RNE) to the mode's 16-bit type, as float32"""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(h16_of(mode)).float().numpy()


# ------------------------------------------------------------------------------------------ the dropout mask (otr_rand32 in numpy)
def rand32(seed, idx):
    s0, s1 = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over='ignore'):
        k0 = np.uint32(s0 * np.uint32(0x9E3779B1)) ^ s1
        k1 = np.uint32(s1 * np.uint32(0x85EBCA77)) ^ np.uint32(s0 >> np.uint32(15)) ^ np.uint32(0xC2B2AE3D)
        x = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ k0
        x = x + ((idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x27D4EB2F))
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x ^= k1
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def keep_mask(c, shift=0):
    """bool [M, d]: the elements dropout keeps; the threshold as the kernel computes it, in float32"""
    M, d = c['M'], c['d']
    if not c['p']:
        return np.ones((M, d), dtype=bool)
    thr = np.uint32(min(int(np.float32(c['p']) * np.float32(4294967296.0)), 4294967295))
    idx = np.uint64(c['rng_offset'] + shift) + np.arange(M * d, dtype=np.uint64)
    return (rand32(SEED, idx) >= thr).reshape(M, d)


def branch_scale(c):
    """s = fp32(fp32(1 / (1 - p)) a_scale), a_scale 0 meaning 1"""
    one = np.float32(1.0)
    inv = one / (one - np.float32(c['p'])) if c['p'] else one
    return np.float32(inv * np.float32(c['a_scale'] or 1.0))


# ------------------------------------------------------------------------------------------ cases
def _case(entry, d, M, at='f', family='unit', **kw):
    c = dict(entry=entry, d=d, M=M, at=at, family=family, p=0.0, a_scale=0.0, has_a=True, mask=family == 'masked', dy16=False, dy3_16=False,
             partial=entry in ('bwd2', 'bwd3'), skip='none', lp_only=False, z_out=True, rng_offset=RNG_OFFSET)
    tag = kw.pop('tag', '')
    c.update(kw)
    assert not (entry in ('bwd2', 'bwd3') and not c['partial']) and not (c['p'] and not c['has_a'])
    nv, tail = D_TABLE[d]
    q, o = M_TABLE[M]
    c['name'] = '%s_d%dnv%d%s_M%dq%do%d_%s_%s%s' % (entry, d, nv, 't' if tail else 'e', M, q, o, at, family, '_' + tag if tag else '')
    return c


def _all_cases():
    out = []
    fw, bw = ('fwd', 'fwd2', 'fwd3'), ('bwd', 'bwd2', 'bwd3')
    for i, d in enumerate(D_TABLE):                         # every d with M = 1 and M = 9, one forward and one backward form each
        out += [_case(fw[i % 3], d, 1, 'fh'[i % 2]), _case(bw[(i + 1) % 3], d, 1, 'hf'[i % 2]),
                _case(fw[(i + 2) % 3], d, 9, 'hf'[i % 2]), _case(bw[i % 3], d, 9, 'fh'[i % 2])]
    for d in (260, 1024):                                   # every M with d = 260 and d = 1024
        for M in M_TABLE:
            out += [_case(e, d, M, 'h', tag='rows') for e in ('fwd', 'fwd3', 'bwd', 'bwd3')]
    for j, d in enumerate((252, 516, 772, 1020)):           # every NV with every form and both `a` types
        for k, e in enumerate(ENTRIES):
            for at in 'fh':
                out.append(_case(e, d, 7, at, tag='nv', p=(0.0, 0.1)[(j + k) % 2], a_scale=(0.0, 0.5)[k % 2], skip=('none', 'sep')[j % 2]))
    for f in FAMILIES:                                      # every family with every form
        for k, e in enumerate(ENTRIES):
            out.append(_case(e, 260, 9, 'fh'[k % 2], f, a_scale=0.5, skip='sep' if e[0] == 'b' else 'none'))
            if f != 'unit':
                out.append(_case(e, 1020, 17, 'hf'[k % 2], f))
    for at in 'fh':                                         # options
        for p in (0.1, 0.5):
            out.append(_case('fwd', 516, 9, at, tag='p%d' % (p * 10), p=p, a_scale=0.5))
            out.append(_case('fwd3', 260, 7, at, tag='p%d_bigoff' % (p * 10), p=p, rng_offset=RNG_OFFSET_BIG))
            for part in (False, True):
                out.append(_case('bwd', 516, 9, at, tag='p%d_%s' % (p * 10, 'part' if part else 'atom'), p=p, a_scale=0.5, partial=part))
            out.append(_case('bwd2', 260, 9, at, tag='p%d' % (p * 10), p=p, skip='alias'))
            out.append(_case('bwd3', 772, 9, at, tag='p%d' % (p * 10), p=p, a_scale=0.5, skip='sep', dy3_16=True))
        for part in (False, True):
            tg = 'part' if part else 'atom'
            out.append(_case('bwd', 260, 17, at, tag='alias_' + tg, skip='alias', partial=part))
            out.append(_case('bwd', 260, 17, at, tag='dy16_' + tg, dy16=True, skip='sep', partial=part))
            out.append(_case('bwd', 1024, 9, at, tag='dy16_' + tg, dy16=True, p=0.1, partial=part))
            out.append(_case('bwd', 260, 9, at, 'masked', tag='p1_' + tg, p=0.1, a_scale=0.5, partial=part))
        out.append(_case('bwd3', 260, 17, at, tag='dy3h_alias', dy3_16=True, skip='alias'))
        out.append(_case('bwd3', 1024, 7, at, 'offset', tag='dy3h', dy3_16=True))
        out.append(_case('fwd', 260, 9, at, tag='lponly', lp_only=True))
        out.append(_case('fwd', 1020, 7, at, 'offset', tag='lponly', lp_only=True, p=0.1))
        out.append(_case('fwd3', 260, 9, at, tag='lponly', lp_only=True))
        out.append(_case('fwd3', 772, 8, at, 'offset', tag='lponly', lp_only=True))
        out.append(_case('fwd', 260, 9, at, tag='noz', z_out=False, a_scale=0.5))
        out.append(_case('fwd', 516, 7, at, 'masked', tag='p1', p=0.1, a_scale=0.5))
    for part in (False, True):                              # no branch at all: a = NULL forward, da = NULL backward
        tg = 'part' if part else 'atom'
        out.append(_case('bwd', 260, 9, 'f', tag='noda_' + tg, has_a=False, partial=part, skip='sep'))
        out.append(_case('bwd', 1020, 17, 'f', 'offset', tag='noda_' + tg, has_a=False, partial=part))
    for e, d in (('fwd', 260), ('fwd2', 516), ('fwd3', 1020), ('bwd2', 260), ('bwd3', 772)):
        out.append(_case(e, d, 9, 'f', tag='noa', has_a=False, skip='alias' if e[0] == 'b' else 'none'))
    by_name = {}
    for c in out:
        by_name.setdefault(c['name'], c)
    return by_name


CASES = _all_cases()
NAMES = tuple(CASES)


def realise(name, mode):
    c = dict(CASES[name], mode=mode)
    c['nblk'] = (c['M'] + 7) // 8
    c['C'] = 4 * ((c['d'] + 255) // 256) + 10
    return c


def prior(d, k):
    """what dgamma (k = 0), dbeta (1), da_colsum (2) hold before an atomics call: known, non-zero"""
    return (0.25 * (k + 1) + 0.001 * np.arange(d)).astype(np.float32)


# ------------------------------------------------------------------------------------------ operands
def _family(g, family, M, d):
    v = g.standard_normal((M, d))
    rows = np.arange(M)
    if family == 'offset':
        v = v + np.where(rows % 2 == 0, 1e3, -1e3)[:, None]
    elif family == 'const':
        v[rows % 3 == 0] = 3.25
        v[rows % 3 == 1] = 0.0
    elif family == 'outlier':
        v[rows, (rows * 37 + d - 1) % d] = 1e4
    elif family == 'tiny':
        v = v * 1e-6
    return v.astype(np.float32)


def _stats(v, eps):
    mu = v.mean(1, keepdims=True)
    var = ((v - mu) ** 2).mean(1, keepdims=True)
    return mu, 1.0 / np.sqrt(var + eps)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _operands(name, mode):
    c = realise(name, mode)
    g = np.random.default_rng(zlib.crc32(name.encode()))
    M, d, fam = c['M'], c['d'], c['family']
    rows = np.arange(M)
    o = {}
    for k in ('1', '2', '3'):
        o['gamma' + k] = (1.0 + 0.2 * g.standard_normal(d)).astype(np.float32)
        o['beta' + k] = (0.2 * g.standard_normal(d)).astype(np.float32)
    o['amask'] = (rows % 3 != 0).astype(np.uint8) if c['mask'] else None
    eps = float(np.float32(EPS))
    if c['entry'][0] == 'f':
        o['x'] = _family(g, fam, M, d)
        a = g.standard_normal((M, d)).astype(np.float32)
        if fam == 'tiny':
            a = a * np.float32(1e-6)
        if fam == 'const':
            a[rows % 3 != 2] = 0.0                              # the constant and the all-zero rows stay what they are in z
        if c['at'] == 'h':
            a = round_h16(a, mode)
        if fam == 'masked':
            bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
            a[o['amask'] == 0] = bad[(np.arange(d) + rows[o['amask'] == 0][:, None]) % 3]
        o['a'] = a if c['has_a'] else None
        return o
    z = _family(g, fam, M, d)
    o['z'] = z
    z64 = z.astype(np.float64)
    mu, r = _stats(z64, eps)
    o['mean'], o['rstd'] = _f32(mu[:, 0]), _f32(r[:, 0])
    if c['entry'] in ('bwd2', 'bwd3'):                          # the later LayerNorms' statistics, of what the kernel recomputes
        y1 = (z64 - o['mean'].astype(np.float64)[:, None]) * o['rstd'].astype(np.float64)[:, None] * o['gamma1'] + o['beta1']
        mu2, r2 = _stats(y1, eps)
        o['mean2'], o['rstd2'] = _f32(mu2[:, 0]), _f32(r2[:, 0])
        y2 = (y1 - o['mean2'].astype(np.float64)[:, None]) * o['rstd2'].astype(np.float64)[:, None] * o['gamma2'] + o['beta2']
        mu3, r3 = _stats(y2, eps)
        o['mean3'], o['rstd3'] = _f32(mu3[:, 0]), _f32(r3[:, 0])
    for k, h in (('dy', c['dy16']), ('dy3', c['dy3_16'])):
        v = g.standard_normal((M, d)).astype(np.float32)
        o[k] = round_h16(v, mode) if h else v
    o['skip'] = g.standard_normal((M, d)).astype(np.float32) if c['skip'] != 'none' else None
    return o


def operands(c):
    """the case's inputs as float32 arrays (16-bit operands hold values of that type); shared, do not write to them"""
    return _operands(c['name'], c['mode'])


# ------------------------------------------------------------------------------------------ float64 reference and bounds
def _ln_fwd(v, din, gamma, beta, eps, C):
    gamma, beta = gamma.astype(np.float64), beta.astype(np.float64)
    mu = v.mean(1, keepdims=True)
    t = v - mu
    var = (t * t).mean(1, keepdims=True)
    r = 1.0 / np.sqrt(var + eps)
    ref = t * r * gamma + beta
    dmu = C * U * np.abs(v).mean(1, keepdims=True) + din.mean(1, keepdims=True)
    dt = U * (np.abs(v) + np.abs(mu)) + dmu + din
    dvar = 2 * (np.abs(t) * dt).mean(1, keepdims=True) + (dt * dt).mean(1, keepdims=True) + C * U * var
    rho = 0.5 * dvar * r * r + 2 * U
    by = dt * r * np.abs(gamma) + np.abs(t * r * gamma) * (rho + 3 * U) + U * np.abs(beta) + U * np.abs(ref)
    return ref, by, (mu[:, 0], (dmu + U * np.abs(mu))[:, 0]), (r[:, 0], (r * rho)[:, 0])


def _ln_bwd(dy, ddy, n, dn, gamma, r, C, U=2 * U):                # (every u of the backward derivation is UB)
    gamma = gamma.astype(np.float64)
    g = dy * gamma
    dg = np.abs(gamma) * ddy + U * np.abs(g)
    s1 = g.mean(1, keepdims=True)
    ds1 = dg.mean(1, keepdims=True) + C * U * np.abs(g).mean(1, keepdims=True)
    s2 = (g * n).mean(1, keepdims=True)
    ds2 = (dg * np.abs(n) + np.abs(g) * dn).mean(1, keepdims=True) + (C + 2) * U * np.abs(g * n).mean(1, keepdims=True)
    out = r * (g - s1 - n * s2)
    dout = r * (dg + ds1 + np.abs(n) * ds2 + np.abs(s2) * dn + 3 * U * (np.abs(g) + np.abs(s1) + np.abs(n * s2))) + 2 * U * np.abs(out)
    tg = dy * n
    return out, dout, (tg, ddy * np.abs(n) + np.abs(dy) * dn + U * np.abs(tg)), (dy, ddy)


def _colsum(c, terms, old):
    t, dt = terms
    ref = t.sum(0) + (old if old is not None else 0.0)
    R = c['M'] + c['nblk'] + 4
    return ref, dt.sum(0) + R * U * (np.abs(old if old is not None else 0.0) + np.abs(t).sum(0))


def _h16_out(c, ref, b, fp32_part=False):
    """the bound of an output that exists in the 16-bit type only: RNE of a value within b of ref (fp16: or half a subnormal step)"""
    if fp32_part:
        return b
    return b * (1 + UH[c['mode']]) + UH[c['mode']] * np.abs(ref) + (2.0 ** -25 if c['mode'] == 'fp16' else 0.0)


def reference(c, got=None, fp32_part=False, o=None):
    """{output: (float64 reference, bound)}.  Forward: y is judged from got['z'], the kernel's own z, when the call returned one.  Backward
    column sums: 'dgamma' .. are old + gradient on the atomics path (old = prior(d, k)), the plain gradient with `partial`.
    fp32_part: the bounds of the 16-bit-only outputs without the rounding to that type (for values that were not rounded yet).
    o: operands in place of the case's own (the autograd-level tests).  A backward whose z / mean / rstd are not stored fp32 inputs but a
    forward kernel's results says how far those may be off, o['dz_in'] [M, d], o['dmean'] / o['drstd'] [M]: the normalised input then
    carries rstd (dz_in + dmean) + |z - mean| drstd on top of its two roundings.  c['old']: what the column sums are added to."""
    o = o if o is not None else operands(c)
    M, d, C = c['M'], c['d'], c['C']
    eps = float(np.float32(EPS))
    s = float(branch_scale(c))
    keep = keep_mask(c)
    rowm = (o['amask'] != 0)[:, None] if o['amask'] is not None else np.ones((M, 1), dtype=bool)
    f = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in o.items()}
    res = {}
    if c['entry'][0] == 'f':
        x = f['x']
        if c['has_a']:
            sa = np.where(rowm & keep, s * np.where(rowm & keep, f['a'], 0.0), 0.0)          # a fill: what a masked row holds is not read
            z = x + sa
            bz = U * (np.abs(x) + 2 * np.abs(sa)) + U * np.abs(z)
        else:
            z, bz = x, np.zeros_like(x)
        res['z'] = (z, bz)
        if got is not None and got.get('z') is not None:
            v, din = got['z'].astype(np.float64), np.zeros_like(z)
        else:
            v, din = z, bz
        y, by, res['mean'], res['rstd'] = _ln_fwd(v, din, o['gamma1'], o['beta1'], eps, C)
        if c['entry'] != 'fwd':
            y, by, res['mean2'], res['rstd2'] = _ln_fwd(y, by, o['gamma2'], o['beta2'], eps, C)
        res['y'] = (y, by)
        if c['entry'] == 'fwd3':
            res['y3'] = _ln_fwd(y, by, o['gamma3'], o['beta3'], eps, C)[:2]
            res['mean3'], res['rstd3'] = _ln_fwd(y, by, o['gamma3'], o['beta3'], eps, C)[2:]
        last = 'y3' if c['entry'] == 'fwd3' else 'y'
        res[last + '16'] = (res[last][0], _h16_out(c, *res[last], fp32_part))
        return res
    col = lambda k: f[k][:, None]
    n = (f['z'] - col('mean')) * col('rstd')
    dn = 2 * UB * np.abs(n)
    if 'dmean' in o:
        dn = dn + col('rstd') * (o['dz_in'] + o['dmean'][:, None]) + np.abs(f['z'] - col('mean')) * o['drstd'][:, None]
    dy, ddy = f['dy'], np.zeros((M, d))
    sums = {}
    if c['entry'] != 'bwd':
        y1 = n * f['gamma1'] + f['beta1']
        dy1 = np.abs(f['gamma1']) * dn + UB * np.abs(n * f['gamma1']) + UB * np.abs(y1)
        n2 = (y1 - col('mean2')) * col('rstd2')
        dn2 = col('rstd2') * (dy1 + UB * np.abs(y1 - col('mean2'))) + UB * np.abs(n2)
        if c['entry'] == 'bwd3':
            y2 = n2 * f['gamma2'] + f['beta2']
            dy2 = np.abs(f['gamma2']) * dn2 + UB * np.abs(n2 * f['gamma2']) + UB * np.abs(y2)
            n3 = (y2 - col('mean3')) * col('rstd3')
            dn3 = col('rstd3') * (dy2 + UB * np.abs(y2 - col('mean3'))) + UB * np.abs(n3)
            g3, dg3, sums['dgamma3'], sums['dbeta3'] = _ln_bwd(f['dy3'], np.zeros((M, d)), n3, dn3, o['gamma3'], col('rstd3'), C)
            dy = dy + g3
            ddy = dg3 + UB * np.abs(dy)
        dy, ddy, sums['dgamma2'], sums['dbeta2'] = _ln_bwd(dy, ddy, n2, dn2, o['gamma2'], col('rstd2'), C)
    dz, ddz, sums['dgamma'], sums['dbeta'] = _ln_bwd(dy, ddy, n, dn, o['gamma1'], col('rstd'), C)
    if f['skip'] is not None:
        dz = dz + f['skip']
        ddz = ddz + UB * np.abs(dz)
    res['dx'] = (dz, ddz)
    if c['has_a']:
        sc = np.where(rowm & keep, s, 0.0)
        da = np.where(sc != 0, dz * sc, 0.0)
        dda = sc * ddz + UB * np.abs(da)
        sums['dacol'] = (da, dda)
        res['da'] = (da, _h16_out(c, da, dda, fp32_part) if c['at'] == 'h' else dda)
    for k, t in sums.items():
        kk = ('dgamma', 'dbeta', 'dacol').index(k) if k in ('dgamma', 'dbeta', 'dacol') else None
        old = prior(d, kk).astype(np.float64) if (kk is not None and not c['partial']) else None
        if 'old' in c:
            old = np.full(d, float(c['old']))
        res[k] = _colsum(c, t, old)
    return res


def ratios(c, got, ref=None):
    """{output: error / bound per element}; NaN where the reference has none, and any other non-finite value, counts as infinite"""
    ref = ref or reference(c, got)
    out = {}
    for k, v in got.items():
        if v is None or k not in ref:
            continue
        r, b = ref[k]
        with np.errstate(all='ignore'):
            q = np.abs(v.astype(np.float64) - r) / np.maximum(b, 1e-300)
        q = np.where(np.isfinite(v) | ~np.isfinite(r), q, np.inf)
        out[k] = np.where(np.isnan(q), np.inf, q)
    return out


def worst(c, rat):
    """(ratio, output, row, column, float4 slot) of the worst element"""
    best = (-1.0, '', -1, -1, -1)
    for k, q in rat.items():
        if q.size == 0:
            continue
        i = int(np.argmax(q))
        val = float(q.flat[i])
        if val > best[0]:
            row, colm = (i // c['d'], i % c['d']) if q.ndim == 2 else ((i, -1) if k.startswith(('mean', 'rstd')) else (-1, i))
            best = (val, k, row, colm, colm // 256 if colm >= 0 else -1)
    return best


# ------------------------------------------------------------------------------------------ fp32 emulation: floor() and the mutants
def _rsum(v, order):
    """row sums of a float32 [M, n] array in float32, in one of three orders"""
    M, n = v.shape
    if n == 0:
        return np.zeros(M, dtype=np.float32)
    if order in ('lane', 'serial'):                            # lane l holds columns (i 64 + l) 4 .. + 3 of slot i, then a 64-lane butterfly
        nv = (n + 255) // 256
        p = np.zeros((M, nv * 256), dtype=np.float32)
        p[:, :n] = v
        p = p.reshape(M, nv, 64, 4)
        acc = np.zeros((M, 64), dtype=np.float32)
        for i in range(nv):
            acc = acc + (((p[:, i, :, 0] + p[:, i, :, 1]) + p[:, i, :, 2]) + p[:, i, :, 3])
        if order == 'serial':                                  # ... or the 64 lane sums one after another
            return np.add.accumulate(acc, axis=1, dtype=np.float32)[:, -1]
    else:
        w = 1 << max(n - 1, 0).bit_length()
        acc = np.zeros((M, w), dtype=np.float32)
        acc[:, :n] = v
    while acc.shape[1] > 1:
        h = acc.shape[1] // 2
        acc = acc[:, :h] + acc[:, h:]
    return acc[:, 0]


def _csum(t, extra=None):
    """column sums in float32, row after row"""
    acc = np.zeros(t.shape[1], dtype=np.float32)
    for r in range(t.shape[0]):
        acc = acc + t[r]
    if extra is not None:
        for r in range(extra[0]):
            acc = acc + extra[1]
    return acc


def emulate(c, order='lane', mutant=None, round16=True):
    """the kernels' arithmetic in float32 numpy; mutant: one of MUTANTS.  The same keys as tests/test_gpu_layernorm.py collects.
    round16=False leaves the 16-bit-only outputs (y16 / y316 of an lp_only case, a 16-bit da) in fp32."""
    o = operands(c)
    M, d = c['M'], c['d']
    f32 = np.float32
    eps, dd = f32(EPS), f32(d)
    nv = (d + 255) // 256
    s = branch_scale(c)
    keep = keep_mask(c, shift=1 if mutant == 'drop_shift' else 0)
    rowm = (o['amask'] != 0)[:, None] if o['amask'] is not None else np.ones((M, 1), dtype=bool)
    sc = np.where(keep, s, f32(0)).astype(f32)
    div = f32(nv * 256) if mutant == 'padded' else dd
    stat = (lambda v: v[:, :d - 4]) if mutant == 'last4' else (lambda v: v)

    def ln(v, gamma, beta):
        mean = _rsum(stat(v), order) / div
        t = v - mean[:, None]
        if mutant == 'onepass':
            var = _rsum(stat(v * v), order) / div - mean * mean
        else:
            var = _rsum(stat(t * t), order) / div
        rstd = f32(1) / np.sqrt(var + (f32(0) if mutant == 'noeps' else eps))
        return t * rstd[:, None] * gamma + beta, mean, rstd

    def bwd(dy, n, gamma, r):
        g = dy * gamma
        s1 = (_rsum(g, order) / dd)[:, None]
        s2 = (_rsum(g * n, order) / dd)[:, None] if mutant != 'no_s2' else f32(0)
        return r * (g - s1 - n * s2), dy * n, dy

    out = {}
    with np.errstate(all='ignore'):
        if c['entry'][0] == 'f':
            z = o['x']
            if c['has_a']:
                a = o['a'] if mutant == 'mask_mul' else np.where(rowm, o['a'], f32(0))      # v += a * sc: one fused multiply-add
                za = (z.astype(np.float64) + a.astype(np.float64) * sc * (rowm if mutant == 'mask_mul' else 1.0)).astype(f32)
                z = za if mutant == 'mask_mul' else np.where(rowm, za, z)
            out['z'] = z if c['z_out'] else None
            y, out['mean'], out['rstd'] = ln(z, o['gamma1'], o['beta1'])
            if c['entry'] != 'fwd':
                y, out['mean2'], out['rstd2'] = ln(y, o['gamma2'], o['beta2'])
            last = 'y'
            out['y'] = y
            if c['entry'] == 'fwd3':
                out['y3'], out['mean3'], out['rstd3'] = ln(y, o['gamma3'], o['beta3'])
                last = 'y3'
            if c['lp_only']:
                v = out.pop(last)
                out[last + '16'] = round_h16(v, c['mode']) if round16 else v
            return out
        col = lambda k: o[k][:, None]
        n = (o['z'] - col('mean')) * col('rstd')
        dy = o['dy']
        ph = ((-M) % 8) if mutant == 'phantom' else 0                # rows of the last workgroup past M, clamped to row M - 1
        terms = {}
        if c['entry'] != 'bwd':
            y1 = n * o['gamma1'] + o['beta1']
            n2 = (y1 - col('mean2')) * col('rstd2')
            if c['entry'] == 'bwd3':
                y2 = n2 * o['gamma2'] + (o['beta1'] if mutant == 'beta1' else o['beta2'])
                n3 = (y2 - col('mean3')) * col('rstd3')
                g3, terms['dgamma3'], terms['dbeta3'] = bwd(o['dy3'], n3, o['gamma3'], col('rstd3'))
                dy = dy + g3
            dy, terms['dgamma2'], terms['dbeta2'] = bwd(dy, n2, o['gamma2'], col('rstd2'))
        dz, terms['dgamma'], terms['dbeta'] = bwd(dy, n, o['gamma1'], col('rstd'))
        if o['skip'] is not None:
            dz = dz + o['skip']
        out['dx'] = dz
        if c['has_a']:
            da = dz * sc * rowm.astype(f32) if mutant == 'mask_mul' else np.where(rowm & (sc != 0), dz * sc, f32(0))
            terms['dacol'] = dz if mutant == 'colsum_pre' else da
            out['da'] = round_h16(da, c['mode']) if (c['at'] == 'h' and round16) else da
        for k, t in terms.items():
            v = _csum(t, (ph, t[-1]) if k != 'dacol' else None)
            kk = ('dgamma', 'dbeta', 'dacol').index(k) if k in ('dgamma', 'dbeta', 'dacol') else None
            out[k] = v + prior(d, kk) if (kk is not None and not c['partial']) else v
    return out


def floor(c, order='lane', round16=False):
    """worst error / bound of the plain fp32 emulation: (ratio, output, row, column, slot).  The 16-bit-only outputs are judged before
    their rounding against the fp32 part of their bound: the rounding itself is exact arithmetic, |RNE(v) - v| <= unit roundoff |v|, and
    comes as close to its share of the bound as the data makes it (round16=True judges the rounded values against the whole bound)."""
    got = emulate(c, order, round16=round16)
    return worst(c, ratios(c, got, reference(c, got, fp32_part=not round16)))


def mutant_ratio(c, mutant):
    return worst(c, ratios(c, emulate(c, 'lane', mutant)))


def custom(mode, entry, d, M, at='f', **kw):
    """a realised case outside the list (the autograd-level tests bring their own operands)"""
    c = dict(_case(entry, d, M, at, **kw), mode=mode)
    c['nblk'] = (M + 7) // 8
    c['C'] = 4 * ((d + 255) // 256) + 10
    return c
