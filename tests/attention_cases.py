"""Named cases for the attention kernels (csrc/attention.hip, encattn.hip, encattn96.hip) and the float64 reference they are judged
by.  No GPU here: tests/test_attention_cases.py checks on the CPU that every case is what its name says, tests/test_gpu_attention.py
runs them through otr_attention_fwd / _bwd / _bias_fwd / _bias_bwd.

The entries dispatch on element type, head dim (16 / 32 / 64 / 96 / 128), operand alignment (`vec_ok`: 16-byte chunks, else the scalar
loaders), waves per workgroup, the merged or split backward and the kind of score bias.  The cases walk that grid at the sizes where
the kernels change path: a second key block with 6 keys, a second 128-query block with 2 rows, utterances without a live key, a first
key block that is wholly masked, masks with holes, Tq or Tk of 1, and the relative-position bias on either side of T = 32 / 33.

reference() is the operation from a materialised score matrix in float64 on the CPU, on the operands as the kernel receives them
(already rounded to the compute type); floor() is the same computation in a plain emulation of the working precision.  Both are
judged blockwise: one 2-norm per (utterance, head, 16 consecutive rows), so that one wrong tile in one head cannot hide in a norm
over the whole tensor."""
import functools
import math
import zlib

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
MODES = ('fp32', 'bf16', 'fp16')
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
TOL = {'fp32': 2e-5, 'bf16': 1.5e-2, 'fp16': 2e-3}          # tests/test_gpu_ops.py: forward; twice that for gradients
BLOCK = 16                                                   # rows of one MFMA tile: what one wave owns
FORWARD = ('out', 'lse')
GRADS = ('delta', 'dq', 'dk', 'dv', 'dbias', 'dbias_h16')
PAD_BIAS = 1.0e4                                             # the padding columns of a relative-position bias: never a score


def h16_of(mode):
    """the library's 16-bit type in this mode (fp32 mode keeps the bf16 build loaded)"""
    return torch.float16 if mode == 'fp16' else torch.bfloat16


# ------------------------------------------------------------------------------------------ builders
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)


def prefix_mask(lens, Tk):
    m = torch.zeros(len(lens), Tk, dtype=torch.uint8)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


def _case(name, family, B, H, Tq, Tk, dk, causal=False, key_mask=None, lay=None, bias=None, key_mask2=None, tensors=None, **claims):
    """q, do [B, Tq, H dk], k, v [B, Tk, H dk] f32 masters (randn * 0.7 as tests/test_gpu_ops.py; the upstream gradient randn);
    lay[x] = (off, bs, ts): operand x starts `off` elements after a 16-byte boundary and is addressed by (batch, time) strides in
    elements, the gradients dq / dk / dv / do with the strides and offset of q / k / v / o as the C ABI has it."""
    g = _gen(name)
    d = H * dk
    c = dict(name=name, family=family, B=B, H=H, Tq=Tq, Tk=Tk, dk=dk, d=d, causal=bool(causal), key_mask=key_mask, key_mask2=key_mask2,
             q=torch.randn(B, Tq, d, generator=g) * 0.7, k=torch.randn(B, Tk, d, generator=g) * 0.7,
             v=torch.randn(B, Tk, d, generator=g) * 0.7, do=torch.randn(B, Tq, d, generator=g), bias=None, rel_shift=0)
    c.update({n: t.float() for n, t in (tensors or {}).items() if n in ('q', 'k', 'v', 'do')})
    base = {'q': (0, Tq * d, d), 'k': (0, Tk * d, d), 'v': (0, Tk * d, d), 'o': (0, Tq * d, d)}
    base.update(lay or {})
    c['lay'] = base
    if bias == 'rel':                                    # [B, T, H, Pp] as ops.RelPosAttentionFn lays it out: 2T - 1 columns padded to 8
        assert Tq == Tk
        P = 2 * Tq - 1
        Pp = (P + 7) // 8 * 8
        t = torch.randn(B, Tq, H, Pp, generator=g) * 2.0
        t[..., P:] = PAD_BIAS
        if tensors and 'bias' in tensors:
            t[..., :P] = tensors['bias'].float()
        c.update(bias=t, rel_shift=1, bias_strides=(Tq * H * Pp, Pp, H * Pp), ncol=Pp)
    elif bias == 'plain':                                # [B, H, Tq, Tk]
        c.update(bias=torch.randn(B, H, Tq, Tk, generator=g) * 2.0, rel_shift=0, bias_strides=(H * Tq * Tk, Tq * Tk, Tk), ncol=Tk)
    c['claims'] = dict(dict(aligned=True, dead=[], bias_vec4=False), **claims)
    return c


def _sweep():
    """every head dim, aligned and in the two unaligned flavours; T = 70: two key blocks, the second with 6 keys, a partly filled
    query block; H B = 9 leaves seven padding workgroups per block row of the XCD-aware grid"""
    out = {}
    B, H, T = 3, 3, 70
    for dk in (16, 32, 64, 96, 128):
        d = H * dk
        for flavour in ('aligned', 'off1', 'stride'):
            lay = None
            if flavour == 'off1':                        # q, k, v, o (and with them every gradient) one element past a 16-byte boundary
                lay = {x: (1, T * d, d) for x in 'qkvo'}
            elif flavour == 'stride':                    # a row stride that is no multiple of the 16-byte chunk (4 fp32 / 8 16-bit elements)
                lay = {x: (0, T * (d + 1), d + 1) for x in 'qkvo'}
            name = 'sweep_d%d_%s' % (dk, flavour)
            out[name] = functools.partial(_case, name, 'sweep', B, H, T, T, dk, key_mask=prefix_mask([70, 41, 57], T), lay=lay,
                                          aligned=flavour == 'aligned')
    return out


def _causal():
    """T = 130: in 16 bits at head dim 64 two 128-query blocks, the second with two rows (fp32: the 64-query blocks, the third with
    two); 200 = 128 + 72.  Ragged: the shortest utterance has ONE live key, which under the causal mask every row still sees."""
    out = {}
    B, H = 3, 2
    for T, dk in ((130, 64), (200, 64), (130, 32)):
        for ragged in (False, True):
            name = 'causal_t%d_d%d%s' % (T, dk, '_ragged' if ragged else '')
            km = prefix_mask([T, T // 2 + 3, 1], T) if ragged else None
            out[name] = functools.partial(_case, name, 'causal', B, H, T, T, dk, causal=True, key_mask=km)
    return out


def _mask_edges():
    out = {}
    B, H, T = 3, 2, 130
    for dk in (64, 32):
        dead = prefix_mask([T, 0, 77], T)                                   # utterance 1 has no live key
        first = torch.ones(B, T, dtype=torch.uint8)
        first[0, :64] = 0                                                   # the running max is still -inf at the first rescale
        first[2, :64] = 0
        first[2, 120:] = 0
        alt = torch.zeros(B, T, dtype=torch.uint8)
        alt[0, 0::2] = 1
        alt[1, 1::2] = 1
        alt[2, 0::3] = 1
        mid = torch.ones(B, T, dtype=torch.uint8)
        mid[0, 64:128] = 0                                                  # keys 128, 129 are live again
        mid[2, 64:128] = 0
        mid[2, :5] = 0
        for tag, km, claims in (('dead', dead, dict(dead=[1])), ('first_block', first, {}), ('alternating', alt, {}), ('middle_block', mid, {})):
            name = 'mask_%s_d%d' % (tag, dk)
            out[name] = functools.partial(_case, name, 'mask', B, H, T, T, dk, key_mask=km, **claims)
    return out


def _cross():
    out = {}
    B, H = 3, 2
    for Tq, Tk in ((130, 70), (1, 1), (70, 1), (1, 200), (5, 49), (64, 65)):
        for dk in (64, 32):
            name = 'cross_%dx%d_d%d' % (Tq, Tk, dk)
            km = prefix_mask([Tk, max(1, Tk // 2), max(1, Tk - 7)], Tk)
            out[name] = functools.partial(_case, name, 'cross', B, H, Tq, Tk, dk, key_mask=km)
    Tq, Tk, dk = 5, 49, 64
    d = H * dk
    km = prefix_mask([Tk, Tk // 2, Tk - 7], Tk)
    # k and v as column slices of a [B, Tk, 6 d] tensor (three layers' k | v: the layout of ops.CrossAttentionSliceFn), layer 1
    lay = {'k': (2 * d, Tk * 6 * d, 6 * d), 'v': (3 * d, Tk * 6 * d, 6 * d)}
    out['cross_kv_slices'] = functools.partial(_case, 'cross_kv_slices', 'cross', B, H, Tq, Tk, dk, key_mask=km, lay=lay)
    Tq, Tk = 70, 130
    km = prefix_mask([Tk, Tk // 2, Tk - 7], Tk)
    lay = {'q': (0, (Tq + 3) * d, d), 'o': (0, (Tq + 1) * d, d)}               # batch strides wider than T * ts
    out['cross_wide_batch_stride'] = functools.partial(_case, 'cross_wide_batch_stride', 'cross', B, H, Tq, Tk, dk, key_mask=km, lay=lay)
    return out


def _bias():
    """rel_shift = 1: T = 20, 32 take the scalar clamped loads, 33 is the first T whose rows are long enough for the 16-byte loads;
    the last utterance is masked past 4/5 of its keys, and key_mask2 is the mask of a second launch on the same gradient buffer"""
    out = {}
    B, H = 2, 3
    for T in (20, 32, 33, 70, 130):
        for dk in (16, 64, 96):
            name = 'bias_rel_t%d_d%d' % (T, dk)
            km = prefix_mask([T, T - T // 5], T)
            km2 = prefix_mask([T - T // 3, T], T)
            out[name] = functools.partial(_case, name, 'bias', B, H, T, T, dk, key_mask=km, key_mask2=km2, bias='rel', bias_vec4=T >= 33)
    for dk in (16, 64):
        name = 'bias_plain_70x130_d%d' % dk
        km = prefix_mask([130, 104], 130)
        km2 = prefix_mask([87, 130], 130)
        out[name] = functools.partial(_case, name, 'bias', B, H, 70, 130, dk, key_mask=km, key_mask2=km2, bias='plain')
    return out


BUILDERS = {}
for _f in (_sweep, _causal, _mask_edges, _cross, _bias):
    BUILDERS.update(_f())
NAMES = list(BUILDERS)
FAMILIES = ('sweep', 'causal', 'mask', 'cross', 'bias')
MASK2 = '/mask2'


def make_case(name, *args, **kw):
    """a case outside the named ones, built from given tensors (tensors = {'q', 'k', 'v', 'do', 'bias' [B, T, H, 2T - 1]}); it is
    not registered: hand it to compute()"""
    return _case(name, 'adhoc', *args, **kw)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`; `name + '/mask2'` is the same case under its second key mask"""
    if name.endswith(MASK2):
        c = dict(build(name[:-len(MASK2)]))
        assert c['key_mask2'] is not None
        c.update(name=name, key_mask=c['key_mask2'])
        return c
    return BUILDERS[name]()


# ------------------------------------------------------------------------------------------ what a case claims
def dead_utterances(c):
    if c['key_mask'] is None:
        return []
    return [b for b in range(c['B']) if int(c['key_mask'][b].sum()) == 0]


def vec_ok(c, mode):
    """attention.hip's vec_ok restated: every batch / time stride and the head dim a multiple of the 16-byte chunk (4 fp32 or 8
    16-bit elements) and every base pointer on a 16-byte boundary"""
    es = 4 if mode == 'fp32' else 2
    ce = 16 // es
    lay = c['lay']
    return all(lay[x][1] % ce == 0 and lay[x][2] % ce == 0 and (lay[x][0] * es) % 16 == 0 for x in 'qkvo') and c['dk'] % ce == 0


def bias_vec4(c):
    """attention.hip's set_bias restated: under rel_shift the 16-byte bias loads of row i run to column 64 ceil(Tk / 64) - 1 + T - 1 - i;
    they are used when, at the corners of (head, row), that stays inside the 2T - 1 columns the strides say are there"""
    if c['bias'] is None or not c['rel_shift']:
        return False
    _, hs, rs = c['bias_strides']
    T, H = c['Tq'], c['H']
    k64 = (c['Tk'] + 63) // 64 * 64
    extent = max(h * hs + i * rs + 2 * T - 1 for h in (0, H - 1) for i in (0, T - 1))
    reach = max(h * hs + i * rs + (k64 - 1) + (T - 1 - i) + 1 for h in (0, H - 1) for i in (0, T - 1))
    return reach <= extent


def owned(lay, B, T, d):
    """(base element, length, bool[length] owned) of the smallest buffer that holds an operand laid out as lay = (off, bs, ts), counted
    from the 16-byte boundary `off` refers to: everything not owned is a guard or a gap that padded strides leave"""
    off, bs, ts = lay
    n = off + (B - 1) * bs + (T - 1) * ts + d
    m = torch.zeros(n, dtype=torch.bool)
    m[off:].as_strided((B, T, d), (bs, ts, 1)).fill_(True)
    return off, n, m


# ------------------------------------------------------------------------------------------ reference
def operands_of(c, mode):
    """q, k, v, do rounded to the compute type of `mode`: what the kernel receives"""
    return {x: c[x].to(DTYPES[mode]) for x in ('q', 'k', 'v', 'do')}


@functools.lru_cache(maxsize=None)
def operands(name, mode):
    return operands_of(build(name), mode)


def heads(x, H):
    """[B, T, H dk] -> [B, H, T, dk]"""
    B, T, d = x.shape
    return x.reshape(B, T, H, d // H).permute(0, 2, 1, 3)


def admissible(c):
    """bool [B, 1, Tq, Tk]: key j may be seen by query i -- key_mask[b, j] != 0, and j <= i under the causal mask (the header)"""
    B, Tq, Tk = c['B'], c['Tq'], c['Tk']
    a = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if c['key_mask'] is not None:
        a = a & (c['key_mask'] != 0).view(B, 1, 1, Tk)
    if c['causal']:
        a = a & (torch.arange(Tk).view(1, Tk) <= torch.arange(Tq).view(Tq, 1)).view(1, 1, Tq, Tk)
    return a


def bias_columns(c):
    """int64 [Tq, Tk]: the column of the bias row i that pair (i, j) reads: j, or j - i + Tq - 1 under rel_shift"""
    i = torch.arange(c['Tq']).view(-1, 1)
    j = torch.arange(c['Tk']).view(1, -1)
    return (j - i + c['Tq'] - 1) if c['rel_shift'] else j.expand(c['Tq'], c['Tk'])


def dense_bias(c):
    """the bias as a [B, H, Tq, Tk] matrix (f32 values)"""
    if not c['rel_shift']:
        return c['bias']
    B, H, Tq, Tk = c['B'], c['H'], c['Tq'], c['Tk']
    col = bias_columns(c).view(1, Tq, 1, Tk).expand(B, Tq, H, Tk)
    return torch.gather(c['bias'], 3, col).permute(0, 2, 1, 3)


def scatter_bias_grad(c, ds):
    """[B, H, Tq, Tk] pair gradients -> the bias tensor's own layout, canonical [B, H, Tq, ncol]; never-read entries are zero"""
    if not c['rel_shift']:
        return ds
    B, H, Tq, Tk = c['B'], c['H'], c['Tq'], c['Tk']
    out = torch.zeros(B, H, Tq, c['ncol'], dtype=ds.dtype)
    out.scatter_(3, bias_columns(c).view(1, 1, Tq, Tk).expand(B, H, Tq, Tk), ds)
    return out


def bias_canonical(c, t):
    """a tensor in the bias' memory layout -> canonical [B, H, Tq, ncol]"""
    return t.permute(0, 2, 1, 3) if c['rel_shift'] else t


def in_band(c):
    """bool [Tq, ncol]: the entries of a bias row that some in-range pair (i, j) reads"""
    m = torch.zeros(c['Tq'], c['ncol'], dtype=torch.bool)
    m.scatter_(1, bias_columns(c), torch.ones(c['Tq'], c['Tk'], dtype=torch.bool))
    return m


def compute(c, mode, emulate):
    """The attention of the case c from a materialised score matrix.  emulate = False: float64 throughout.  emulate = True: the
    working precision of the kernels, plainly -- inputs in the compute type, scores / softmax / accumulation in float32, P and dS
    rounded to the compute type before their products, outputs rounded to the compute type (lse, delta and dbias are f32 outputs).

    A query row with no admissible key: out = 0, lse = -inf, P = 0 and with it every gradient contribution; masked keys get
    dk = dv = 0 and masked pairs dbias = 0 because their P is 0."""
    H, dk = c['H'], c['dk']
    ct = DTYPES[mode]
    wt = torch.float32 if emulate else torch.float64
    rnd = (lambda x: x.to(ct).to(wt)) if emulate else (lambda x: x)
    x = operands_of(c, mode)
    q, k, v, do = (heads(x[n].to(wt), H) for n in ('q', 'k', 'v', 'do'))
    scale = float(torch.tensor(1.0 / math.sqrt(dk), dtype=torch.float32))        # the float the descriptor carries
    s = q @ k.transpose(-1, -2)
    if c['bias'] is not None:
        s = s + dense_bias(c).to(wt)
    s = s * scale
    adm = admissible(c).expand(c['B'], H, c['Tq'], c['Tk'])
    live = adm.any(-1, keepdim=True)
    ninf = torch.full((), float('-inf'), dtype=wt)
    zero = torch.zeros((), dtype=wt)
    sm = torch.where(adm, s, ninf)
    m = torch.where(live, sm.max(-1, keepdim=True).values, zero)
    e = torch.exp(sm - m)
    l = e.sum(-1, keepdim=True)
    lse_f = torch.where(live, m + torch.log(l.clamp_min(1e-300 if not emulate else 1e-38)), zero)      # finite stand-in on dead rows
    p_fwd = torch.where(live, e / torch.where(live, l, torch.ones((), dtype=wt)), zero)
    out = rnd(rnd(p_fwd) @ v)
    p = torch.where(adm & live, torch.exp(sm - lse_f), zero)                      # as the backward kernels recompute it
    delta = (do * out).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - delta) * scale                                                 # d loss / d (q.k + bias)
    dsr = rnd(ds)
    res = {'out': out, 'lse': torch.where(live, lse_f, ninf), 'delta': delta, 'dq': rnd(dsr @ k), 'dk': rnd(dsr.transpose(-1, -2) @ q),
           'dv': rnd(rnd(p).transpose(-1, -2) @ do)}
    if c['bias'] is not None:
        res['dbias'] = scatter_bias_grad(c, ds)
        res['dbias_h16'] = res['dbias'].to(h16_of(mode)).to(wt) if emulate else res['dbias']
    res = {n: t.double() for n, t in res.items()}
    if not emulate:
        res['_p'], res['_s'], res['_adm'] = p, s, adm
    return res


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """float64 {'out', 'dq' [B, H, Tq, dk], 'lse', 'delta' [B, H, Tq, 1], 'dk', 'dv' [B, H, Tk, dk], 'dbias' (= 'dbias_h16')
    [B, H, Tq, ncol]} of the case on its operands rounded to `mode`'s compute type"""
    return compute(build(name), mode, False)


@functools.lru_cache(maxsize=None)
def floor(name, mode):
    """the same in the emulated working precision: its distance from reference() is the noise a correct kernel is entitled to"""
    return compute(build(name), mode, True)


def outputs(c):
    return ['out', 'lse', 'delta', 'dq', 'dk', 'dv'] + (['dbias', 'dbias_h16'] if c['bias'] is not None else [])


# ------------------------------------------------------------------------------------------ distances
def block_norms(x):
    """[B, H, T, W] -> [B, H, ceil(T / 16)]: the 2-norm of every block of 16 consecutive rows"""
    B, H, T, W = x.shape
    nb = (T + BLOCK - 1) // BLOCK
    pad = torch.zeros(B, H, nb * BLOCK, W, dtype=x.dtype)
    pad[:, :, :T] = x
    return pad.view(B, H, nb, BLOCK * W).norm(dim=-1)


def diff(a, ref):
    """a - ref in float64 with equal infinities counting as no difference (lse of a dead row); a NaN stays one"""
    a, ref = a.double(), ref.double()
    return torch.where(a == ref, torch.zeros_like(ref), a - ref)


def distances(a, ref):
    """(blockwise distance [B, H, nb], whole-tensor Frobenius distance, Frobenius norm of ref over its finite entries)"""
    d = diff(a, ref)
    n = float(torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref)).norm())
    return block_norms(d), float(d.norm()), n


def tol_of(output, mode):
    """the whole-tensor tolerance of tests/test_gpu_ops.py: TOL for what the forward pass writes, twice that for gradients; a bias
    gradient taken in 16 bits is held to the tolerance of that type in every mode (fp32 mode writes it as bf16)"""
    if output == 'dbias_h16':
        return 2.0 * TOL['fp16' if mode == 'fp16' else 'bf16']
    return TOL[mode] * (1.0 if output in FORWARD else 2.0)


def whole_ok(output, mode, dist, ref_norm, tiny_blocks, floor_dist, K):
    """The whole-tensor check: |a - ref| <= TOL |ref|, the relative Frobenius bound of tests/test_gpu_ops.py.  Where the reference is
    degenerate -- its norm below the tensor's tiny, i.e. below one float32 rounding of its own terms: dq and dk at Tk = 1, zero in
    exact arithmetic -- a relative bound says nothing and the absolute |a - ref| <= K |floor - ref| + |tiny| stands in."""
    t = float(tiny_blocks.norm())
    if ref_norm <= t:
        return dist <= K * floor_dist + t
    return dist <= tol_of(output, mode) * ref_norm


@functools.lru_cache(maxsize=None)
def floor_distances(name, mode):
    ref, fl = reference(name, mode), floor(name, mode)
    return {n: distances(fl[n], ref[n]) for n in outputs(build(name))}


SIGMA_OUTPUTS = ('delta', 'dbias')


@functools.lru_cache(maxsize=None)
def tiny(name, mode):
    """Slack for blocks whose reference is zero or a few ulps, per output and block: next to an ordinary block's floor it is small,
    so that K * floor is the bound there.

    out, dq, dk, dv, dbias: eps_fp32 * |A_block|, A the root of the sum of the SQUARES of the terms of each element's sum (float64):
    sqrt(P^2 v^2) for out, sqrt(P^2^T do^2) for dv, sqrt(|dS|^2 k^2) for dq, sqrt(|dS|^2^T q^2) for dk and |dS| itself for dbias -- one
    float32 rounding on every term, independent.  |dS| = scale P (sum_c |do_c v_c| + sum_c |do_c o_c|): the two inner sums over the
    head dim, dP and delta, enter by their difference, whose error is one rounding at the size of their partial sums (as for delta
    below), not of one term.  It matters where a block is zero in exact arithmetic: with one live key P is 1, out is v and
    dP - delta = 0, so dq, dk and dbias cancel to nothing in float64 -- and in a float32 emulation that forms both sums the same way
    (Tq = Tk = 1: the floor is exactly 0) -- and to a rounding of those sums in a kernel that forms them in two different orders.

    lse and delta are ONE number per row, so a block with two rows (T = 130) or one (Tq = 1) holds one or two rounding draws and the
    floor's own draw can be a twentieth of the typical size.  Their slack is therefore a rounding count, not a share of the floor:
    delta: eps_fp32 * sum_c |do_c o_c|, one rounding at the size of the partial sums; lse: 4 eps_fp32 (1 + |lse|), the roundings
    of m + log(l) (the score s at the size of |lse|, its scaling, the logarithm, the sum).

    delta and the fp32 dbias, 16-bit modes only: + 4 sigma_i, sigma_i = u |do_i o_i|_2 / sqrt(3), u = eps of the compute type / 2.
    delta_i = sum_c do_ic o_ic is formed from the ROUNDED o, each element off by an independent error uniform in +- u |o_ic|, of
    standard deviation u |o_ic| / sqrt(3): delta_i carries one draw of standard deviation sigma_i, and four of them bound a draw
    that is not a defect.  The same draw scales dS_ij = scale P_ij (dP_ij - delta_i) of its whole row, which is the fp32 dbias.
    dq, dk and the 16-bit dbias average it over many terms or round it away and get no such term."""
    c = build(name)
    ref = reference(name, mode)
    H = c['H']
    x = operands(name, mode)
    q, k, v, do = (heads(x[n].double(), H) for n in ('q', 'k', 'v', 'do'))
    p = ref['_p']
    scale = float(torch.tensor(1.0 / math.sqrt(c['dk']), dtype=torch.float32))
    do_o = do * ref['out']
    a_ds = scale * p * (do.abs() @ v.abs().transpose(-1, -2) + do_o.abs().sum(-1, keepdim=True))
    lse = ref['lse']
    A = {'out': ((p ** 2) @ (v ** 2)).sqrt(), 'lse': 4.0 * torch.where(torch.isfinite(lse), 1.0 + lse.abs(), torch.zeros_like(lse)),
         'delta': do_o.abs().sum(-1, keepdim=True), 'dq': ((a_ds ** 2) @ (k ** 2)).sqrt(),
         'dk': ((a_ds ** 2).transpose(-1, -2) @ (q ** 2)).sqrt(), 'dv': ((p ** 2).transpose(-1, -2) @ (do ** 2)).sqrt()}
    u = 0.0 if mode == 'fp32' else float(torch.finfo(DTYPES[mode]).eps) / 2
    d_delta = 4.0 / math.sqrt(3.0) * u * do_o.norm(dim=-1, keepdim=True)                             # [B, H, Tq, 1]
    D = {'delta': d_delta}
    if c['bias'] is not None:
        A['dbias'] = A['dbias_h16'] = scatter_bias_grad(c, a_ds)
        D['dbias'] = scatter_bias_grad(c, scale * p * d_delta)
    return {n: EPS32 * block_norms(t) + (block_norms(D[n]) if n in D else 0.0) for n, t in A.items()}
