"""GPU (-m gpu): otr_attention_fwd / _bwd / _bias_fwd / _bias_bwd through the C ABI against float64 on the CPU, per block of 16 rows.

The cases (tests/attention_cases.py, checked on the CPU by tests/test_attention_cases.py) are run in fp32, bf16 and fp16 with every
output inside a guarded buffer: the guards and the gaps that padded strides leave must not change, every owned element must have been
written.  out, lse, delta, dq, dk, dv and dbias are held to  err_block <= K * floor_block + tiny_block  per (utterance, head, 16 rows)
and to the plain whole-tensor tolerances of tests/test_gpu_ops.py; dead rows, masked keys and masked bias pairs must be exact zeros.

Routing (otr_attention_fwd, attention_bwd_impl; `vec` = vec_ok, `16` = bf16 / fp16):
  forward   vec, 16, head dim 64                      attn_fwd_kernel<16, 64, PIPE, 8 waves>     sweep_d64_aligned, causal_*_d64, mask_*_d64,
                                                                                                 cross_*_d64, bias_*_d64
            vec, anything else                        attn_fwd_kernel<T, dk, PIPE, 4 waves>      every other aligned case; all of fp32
            not vec                                   attn_fwd_kernel<T, dk, no PIPE, 4 waves>   sweep_*_off1, sweep_*_stride (load_tile_rm / _tr,
                                                                                                 the scalar branch of store4)
  backward  vec, 16, dk 96, rel_shift, bias_vec4,     encattn96.hip (key 33 = 0 turns it off)    bias_rel_t33 / t70 / t130_d96
              dbias, Tq = Tk <= 512, not causal
            vec, 16, dk 64, no bias, Tq = Tk <= 512,  encattn.hip (key 21 = 0 turns it off)      sweep_d64_aligned, mask_*_d64
              not causal
            vec, 16 and dk <= 64, or fp32 and         attn_bwd_kernel (merged; 8 waves for 16    the above with 21 = 0, causal_*, cross_* (aligned),
              dk <= 32 (key 13 = 1 turns it off)        bit dk 64, else 4)                       bias_*_d16 / d64, sweep_d16 / d32_aligned
            otherwise                                 attn_bwd_dq_kernel + attn_bwd_dkdv_kernel  16 bit dk 96 / 128, fp32 dk 64 / 96 / 128, every
                                                        (PIPE iff vec)                           unaligned case, and all of the above with 13 = 1
  bias      rel_shift, T <= 32                        scalar clamped loads (bias_vec4 = 0)       bias_rel_t20, bias_rel_t32
            rel_shift, T >= 33                        bias_load4                                 bias_rel_t33, t70, t130
            rel_shift = 0                             scalar clamped loads                       bias_plain_70x130
Every backward form a case can take is run (backward_forms restates the dispatch); every test writes the figures it measured into
parity_out/attention_parity.json (or under $OTR_PARITY_DIR) before it asserts.

K.  err_block / floor_block, worst over the ordinary blocks (reference above its tiny, i.e. not zero in exact arithmetic), measured on
MI355X over every case, backward form and launch of this module.  In brackets: the largest share of K * floor + tiny that is used.
                  out           dq dk dv dbias16   lse            delta          dbias f32
  sweep   fp32    1.38 (0.27)   2.58 (0.21)        4.62 (0.14)    4.99 (0.29)
          bf16    1.12 (0.37)   1.25 (0.25)        5.96 (0.14)    4.15 (0.27)
          fp16    1.27 (0.42)   1.22 (0.24)        5.12 (0.13)    2.61 (0.24)
  causal  fp32    1.45 (0.32)   6.63 (0.50)        6.08 (0.15)    6.47 (0.31)
          bf16    1.10 (0.37)   1.47 (0.29)        9.73 (0.15)   24.60 (0.36)
          fp16    1.18 (0.40)   1.35 (0.27)        5.97 (0.17)    4.45 (0.26)
  mask    fp32    1.43 (0.30)   1.89 (0.16)       13.80 (0.15)   29.10 (0.38)
          bf16    1.24 (0.41)   1.20 (0.24)       34.50 (0.18)    8.27 (0.27)
          fp16    1.14 (0.38)   1.37 (0.27)       20.70 (0.18)    5.35 (0.29)
  cross   fp32    1.71 (0.36)   8.90 (0.37)       15.80 (0.18)   33.00 (0.71)
          bf16    1.19 (0.40)   1.20 (0.24)       14.70 (0.19)    4.94 (0.22)
          fp16    1.28 (0.42)   2.47 (0.49)       31.00 (0.18)   32.90 (0.32)
  bias    fp32    1.49 (0.32)   3.90 (0.31)       11.80 (0.13)   19.60 (0.51)    6.03 (0.43)
          bf16    1.27 (0.42)   1.41 (0.28)       17.50 (0.18)    6.83 (0.32)    6.85 (0.31)
          fp16    1.24 (0.41)   1.61 (0.32)       15.40 (0.15)   14.20 (0.55)   14.10 (0.55)
The brackets were taken with K = 10 for the fp32 gradients; under the K below they grow by at most 1.25.
out: worst 1.71 in fp32 and 1.28 in 16 bits: K = 4 and 3.  dq, dk, dv, 16-bit dbias: 2.47 in 16 bits, K = 5.  In fp32 3.90 over the
blocks whose elements are sums of many terms, K = 8.  The fp32 figures above that, 5.76 .. 8.90, are NOT adopted: they are the
blocks of sums of one or two terms -- dk and dv at Tq = 1 (dv_j = P_j do), and the last keys under the causal mask, seen by one or
two queries -- where the floor is the single rounding of P and the kernel's P carries the roundings of its exponent s - lse at the
size of |s| + |lse|; they use at most 0.60 of the bound under K = 8.
lse, delta and the fp32 dbias are not adopted into K either.  lse_i and delta_i are one number per row, so the last block of T = 130,
33 or 70 (two, one, six rows) and Tq = 1 hold a few draws of a rounding error and the floor's own draw can be a thirtieth of the
typical size: the ratio measures the floor's luck.  What bounds them is the rounding count of attention_cases.tiny (4 ulp of
1 + |lse|; one rounding at the size of delta's partial sums; in 16 bits four standard deviations of the rounding of o), of which
the kernels use at most 0.19 for lse and 0.75 for delta.  dbias in fp32 inherits delta's draw through dS = scale P (dP - delta).
Five mutations of csrc/attention.hip were run against this module, each fails it: no m_safe guard in the forward (mask_dead_*,
mask_first_block_*: NaN); the dK tiles of two waves of one head swapped (every case with Tk >= 32: that block at 1e+0 against a floor
of 1e-7, the whole-tensor distance 0.28); the bias read at column j under rel_shift (every bias_rel case); no zero store for a masked
bias pair (bias_plain: entries left unwritten; every second launch of test_rel_shift_gradient_tensor_kept_across_steps: stale values);
vec_ok ignoring the base pointers (sweep_d64_off1 in 16 bits goes to csrc/encattn.hip and leaves the delta workspace unwritten where
the streamed kernels are expected -- misaligned vector loads return correct data, so only the routing shows it)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import attention_cases as ac

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = {'fp32': {'fwd': 4.0, 'grad': 8.0}, 'bf16': {'fwd': 3.0, 'grad': 5.0}, 'fp16': {'fwd': 3.0, 'grad': 5.0}}
GUARD = 64                    # elements before and after every buffer: a multiple of 16 bytes in every type
SENTINEL = 1234.0
DEFAULTS = {33: 1, 21: 1, 13: 0}
REPORT = {}


def _report(key, rec):
    REPORT[key] = rec
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'attention_parity.json'), 'w') as f:
        json.dump(json.loads(json.dumps(REPORT), parse_float=lambda x: float('%.3g' % float(x))), f, sort_keys=True, indent=None,
                  separators=(',', ':'))


@pytest.fixture(params=ac.MODES)
def mode(request):
    from opentransformer_amd import ops
    ops.set_compute_dtype(request.param)
    yield request.param
    ops.set_compute_dtype('bf16')


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """an operand laid out as lay = (off, bs, ts) inside a buffer with GUARD elements on either side; everything but the owned
    elements holds SENTINEL, the owned ones start as `fill` (NaN for an output)"""

    def __init__(self, lay, B, T, d, dtype, fill=float('nan'), value=None):
        off, n, own = ac.owned(lay, B, T, d)
        self.shape, self.strides, self.base = (B, T, d), (lay[1], lay[2], 1), GUARD + off
        self.own = torch.zeros(n + 2 * GUARD, dtype=torch.bool)
        self.own[GUARD:GUARD + n] = own
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        if value is not None:
            self.view().copy_(value.to(DEV))
        else:
            self.view().fill_(fill)
        self.before = self.buf.clone()

    def view(self):
        return self.buf[self.base:].as_strided(self.shape, self.strides)

    def ptr(self):
        return _p(self.buf, self.base)

    def check(self, what, written=True):
        """guards and gaps unchanged; every owned element finite (so: written, it started as NaN)"""
        now = self.buf.cpu()
        keep = ~self.own
        assert torch.equal(now[keep], self.before.cpu()[keep]), what + ('guard or gap overwritten',)
        if written:
            bad = ~torch.isfinite(now[self.own].float())
            assert not bool(bad.any()), what + ('%d owned elements not written or not finite' % int(bad.sum()),)


def _flat(shape, dtype, fill):
    """a contiguous tensor as a Guarded with one row"""
    n = 1
    for s in shape:
        n *= s
    return Guarded((0, n, n), 1, 1, n, dtype, fill=fill)


# ------------------------------------------------------------------------------------------ launches
def backward_forms(c, mode):
    """the backward launches this case is given: [(name, {debug key: value}, served by a whole-utterance kernel)] -- attention_bwd_impl
    restated.  The library's own choice comes first, then every other form the shape can take."""
    vec, h16 = ac.vec_ok(c, mode), mode != 'fp32'
    same, dk = c['Tq'] == c['Tk'] <= 512 and not c['causal'], c['dk']
    enc96 = h16 and vec and dk == 96 and same and c['bias'] is not None and bool(c['rel_shift']) and ac.bias_vec4(c)
    enc = h16 and vec and dk == 64 and same and c['bias'] is None
    merged = vec and (dk <= 64 if h16 else dk <= 32)
    forms = [('default: ' + ('encattn96' if enc96 else 'encattn' if enc else 'merged' if merged else 'split'), {}, enc96 or enc)]
    if merged and (enc96 or enc):
        forms.append(('merged', {33: 0, 21: 0}, False))
    if merged or enc96 or enc:
        forms.append(('split', {33: 0, 21: 0, 13: 1}, False))
    return forms


class Run:
    """one case in one mode on the device: forward once, then any number of backward launches"""

    def __init__(self, name, mode):
        from opentransformer_amd import _lib as L, ops
        self.L, self.ops, self.lib = L, ops, L.load()
        self.name, self.mode, self.c = name, mode, ac.build(name)
        c = self.c
        self.adt = ac.DTYPES[mode]
        x = ac.operands(name, mode)
        B, H, Tq, Tk, d = c['B'], c['H'], c['Tq'], c['Tk'], c['d']
        lay = c['lay']
        self.q = Guarded(lay['q'], B, Tq, d, self.adt, value=x['q'])
        self.k = Guarded(lay['k'], B, Tk, d, self.adt, value=x['k'])
        self.v = Guarded(lay['v'], B, Tk, d, self.adt, value=x['v'])
        self.do = Guarded(lay['o'], B, Tq, d, self.adt, value=x['do'])
        self.km = c['key_mask'].to(DEV).contiguous() if c['key_mask'] is not None else None
        self.bias = c['bias'].to(DEV).contiguous() if c['bias'] is not None else None
        self.desc = ops._attn_desc(B, H, Tq, Tk, c['dk'], self.adt, lay['q'][1:], lay['k'][1:], lay['v'][1:], lay['o'][1:], c['causal'])
        es = 2 if mode != 'fp32' else 4
        aligned = all(t.ptr().value % 16 == 0 for t in (self.q, self.k, self.v, self.do))
        assert aligned == all((lay[x][0] * es) % 16 == 0 for x in 'qkvo')

    def forward(self):
        c, lib = self.c, self.lib
        B, H, Tq, d = c['B'], c['H'], c['Tq'], c['d']
        self.o = Guarded(c['lay']['o'], B, Tq, d, self.adt)
        self.lse = _flat((B, H, Tq), torch.float32, float('nan'))
        if self.bias is None:
            ret = lib.otr_attention_fwd(C.byref(self.desc), self.q.ptr(), self.k.ptr(), self.v.ptr(), _p(self.km), self.o.ptr(), self.lse.ptr(),
                                        _stream())
        else:
            bs, hs, rs = c['bias_strides']
            ret = lib.otr_attention_bias_fwd(C.byref(self.desc), self.q.ptr(), self.k.ptr(), self.v.ptr(), _p(self.km), _p(self.bias), bs, hs, rs,
                                             c['rel_shift'], self.o.ptr(), self.lse.ptr(), _stream())
        self.L.check(ret, 'attention forward')
        torch.cuda.synchronize()
        where = (self.name, self.mode, 'forward')
        self.o.check(where + ('out',))
        self.lse.check(where + ('lse',), written=False)
        lse = self.lse.view().view(B, H, Tq, 1).cpu()
        assert not bool(torch.isnan(lse).any()) and not bool((lse == float('inf')).any()), where + ('lse not written',)
        for t in (self.q, self.k, self.v):
            t.check(where + ('an input changed',))
        return {'out': ac.heads(self.o.view().cpu().double(), H), 'lse': lse.double()}

    def backward(self, settings, dbias16=False, dbias=None, whole_utterance=False):
        """one backward launch under the debug settings; dbias: a Guarded to reuse (a tensor kept across steps), else a fresh one,
        pre-zeroed under rel_shift as the header asks and NaN otherwise; whole_utterance: encattn.hip / encattn96.hip take this launch,
        which need not write the delta workspace (include/otrans_hip.h)"""
        c, lib = self.c, self.lib
        B, H, Tq, Tk, d = c['B'], c['H'], c['Tq'], c['Tk'], c['d']
        lay = c['lay']
        dq, dk, dv = Guarded(lay['q'], B, Tq, d, self.adt), Guarded(lay['k'], B, Tk, d, self.adt), Guarded(lay['v'], B, Tk, d, self.adt)
        delta = _flat((B, H, Tq), torch.float32, float('nan'))
        if self.bias is not None and dbias is None:
            dbias = _flat(tuple(self.bias.shape), ac.h16_of(self.mode) if dbias16 else torch.float32, 0.0 if c['rel_shift'] else float('nan'))
        try:
            for key, val in {**DEFAULTS, **settings}.items():
                self.L.check(lib.otr_debug_set(key, val), 'otr_debug_set')
            if self.bias is None:
                ret = lib.otr_attention_bwd(C.byref(self.desc), self.q.ptr(), self.k.ptr(), self.v.ptr(), _p(self.km), self.o.ptr(), self.do.ptr(),
                                            self.lse.ptr(), delta.ptr(), dq.ptr(), dk.ptr(), dv.ptr(), _stream())
            else:
                bs, hs, rs = c['bias_strides']
                ret = lib.otr_attention_bias_bwd(C.byref(self.desc), self.q.ptr(), self.k.ptr(), self.v.ptr(), _p(self.km), _p(self.bias), dbias.ptr(),
                                                 self.ops._code(dbias.buf.dtype), bs, hs, rs, c['rel_shift'], self.o.ptr(), self.do.ptr(), self.lse.ptr(),
                                                 delta.ptr(), dq.ptr(), dk.ptr(), dv.ptr(), _stream())
            self.L.check(ret, 'attention backward')
            torch.cuda.synchronize()
        finally:
            for key, val in DEFAULTS.items():
                lib.otr_debug_set(key, val)
        where = (self.name, self.mode, 'backward', json.dumps(settings))
        got = {}
        for n, t in (('dq', dq), ('dk', dk), ('dv', dv)):
            t.check(where + (n,))
            got[n] = ac.heads(t.view().cpu().double(), H)
        # delta is a workspace.  The streamed kernels must leave rowsum(dO * O) in all of it; a whole-utterance kernel need not write it,
        # but then leaves it alone: all of it or none.  This is also how the module sees the routing from outside: a launch that
        # backward_forms expects on the streamed kernels and that leaves delta unwritten went somewhere else.
        if whole_utterance and torch.equal(delta.buf.cpu().view(torch.int32), delta.before.cpu().view(torch.int32)):
            pass
        else:
            delta.check(where + ('delta',))
            got['delta'] = delta.view().view(B, H, Tq, 1).cpu().double()
        for t in (self.q, self.k, self.v, self.o, self.do, self.lse):
            t.check(where + ('an input changed',), written=False)
        if dbias is not None:
            dbias.check(where + ('dbias',))
            got['dbias_h16' if dbias16 else 'dbias'] = ac.bias_canonical(c, dbias.view().view(self.bias.shape).cpu().double())
            self.dbias = dbias
        return got

    def set_mask(self, km):
        self.km = km.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------ judging
def judge(name, mode, tag, got):
    """every output in `got` against reference(): the figures are recorded first, then the exact zeros, the blockwise bound and the
    whole-tensor tolerance are asserted"""
    c = ac.build(name)
    ref, fd, tn = ac.reference(name, mode), ac.floor_distances(name, mode), ac.tiny(name, mode)
    rec, fails = {}, []
    for n, a in got.items():
        blocks, dist, norm = ac.distances(a, ref[n])
        fblocks = fd[n][0]
        k = K[mode]['fwd' if n in ac.FORWARD else 'grad']
        rblocks = ac.block_norms(torch.where(torch.isfinite(ref[n]), ref[n], torch.zeros_like(ref[n])))
        above = (rblocks > tn[n]) & (fblocks > 0)                                       # an ordinary block: not below one rounding of its own terms
        raw = float((blocks / fblocks.clamp_min(1e-300))[above].max()) if bool(above.any()) else 0.0
        raw_any = float((blocks / fblocks.clamp_min(1e-300))[fblocks > 0].max()) if bool((fblocks > 0).any()) else 0.0
        bound = k * fblocks + tn[n]
        usage = float((blocks / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
        rec[n] = {'ratio': raw, 'ratio_any': raw_any, 'usage': usage, 'whole': dist / max(norm, 1e-300), 'floor_whole': fd[n][1] / max(norm, 1e-300)}
        bad = ~(blocks <= bound)                                           # a NaN block is bad
        if bool(bad.any()):
            b, h, blk = [int(i) for i in bad.nonzero()[0]]
            fails.append((n, 'utterance %d head %d rows %d..%d' % (b, h, blk * ac.BLOCK, blk * ac.BLOCK + ac.BLOCK - 1), 'err %.3e floor %.3e tiny %.3e'
                          % (float(blocks[b, h, blk]), float(fblocks[b, h, blk]), float(tn[n][b, h, blk])), '%d blocks' % int(bad.sum())))
        if not ac.whole_ok(n, mode, dist, norm, tn[n], fd[n][1], k):
            fails.append((n, 'whole tensor', dist / max(norm, 1e-300), ac.tol_of(n, mode)))
    _report('%s|%s|%s' % (name, mode, tag), dict(rec, family=c['family']))
    print(name, mode, tag, json.dumps({n: round(r['ratio'], 2) for n, r in rec.items()}))
    # exact structure
    adm = ac.admissible(c)[:, 0]                                                           # [B, Tq, Tk]
    dead = ~adm.any(-1)                                                                    # [B, Tq]
    for n, a in got.items():
        where = (name, mode, tag, n)
        if n == 'lse':
            assert bool((a[:, :, :, 0] == float('-inf'))[dead[:, None, :].expand_as(a[:, :, :, 0])].all()), where + ('lse of a dead row',)
            assert bool(torch.isfinite(a[:, :, :, 0][~dead[:, None, :].expand_as(a[:, :, :, 0])]).all()), where + ('lse of a live row',)
        elif n in ('out', 'delta', 'dq'):
            assert float(a.abs().sum(-1)[dead[:, None, :].expand(a.shape[:3])].sum()) == 0.0, where + ('dead rows',)
        elif n in ('dk', 'dv'):
            unseen = ~adm.any(1)                                                           # [B, Tk]: no query may see this key
            assert float(a.abs().sum(-1)[unseen[:, None, :].expand(a.shape[:3])].sum()) == 0.0, where + ('masked keys',)
        else:
            zero = ac.scatter_bias_grad(c, (~adm)[:, None].expand(c['B'], c['H'], c['Tq'], c['Tk']).double()) != 0     # masked in-range pairs
            assert float(a[zero].abs().sum()) == 0.0, where + ('masked bias pairs',)
            if c['rel_shift']:
                assert float(a[:, :, ~ac.in_band(c)].abs().sum()) == 0.0, where + ('off-band entries and padding columns',)
    assert not fails, (name, mode, tag, fails)


# ------------------------------------------------------------------------------------------ every case, every form
@pytest.mark.parametrize('name', ac.NAMES)
def test_attention_matches_float64(mode, name):
    c = ac.build(name)
    run = Run(name, mode)
    judge(name, mode, 'forward', run.forward())
    forms = backward_forms(c, mode)
    for form, settings, whole in forms:
        judge(name, mode, form, run.backward(settings, whole_utterance=whole))
        if c['bias'] is not None:
            judge(name, mode, form + ' dbias16', run.backward(settings, dbias16=True, whole_utterance=whole))


@pytest.mark.parametrize('name', [n for n in ac.NAMES if ac.build(n)['family'] == 'bias' and ac.build(n)['rel_shift']])
def test_rel_shift_gradient_tensor_kept_across_steps(mode, name):
    """ops.RelPosAttentionFn zeroes the score term's gradient tensor once and keeps it: a second launch under another mask on the
    same buffer, whose band holds the first launch's values plus 7, leaves no stale entry -- every in-band entry is overwritten (masked
    pairs with zero), off-band entries and padding columns stay zero"""
    c = ac.build(name)
    band = ac.in_band(c).view(1, c['Tq'], 1, c['ncol']).to(DEV)
    for form, settings, whole in backward_forms(c, mode):
        for dbias16 in (False, True):
            run = Run(name, mode)
            run.forward()
            first = run.backward(settings, dbias16=dbias16, whole_utterance=whole)
            kept = run.dbias
            assert float(first['dbias_h16' if dbias16 else 'dbias'].abs().sum()) > 0.0
            kept.view().view(run.bias.shape).add_(7.0 * band.to(kept.buf.dtype))
            kept.before = kept.buf.clone()
            run.set_mask(c['key_mask2'])
            run.forward()
            again = run.backward(settings, dbias16=dbias16, dbias=kept, whole_utterance=whole)
            judge(name + ac.MASK2, mode, form + (' dbias16' if dbias16 else '') + ' second launch', again)


# ------------------------------------------------------------------------------------------ through ops
def _one_off(x):
    """x as a view one element into a flat buffer: contiguous, and 2 or 4 bytes past a 16-byte boundary"""
    flat = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    flat[1:1 + x.numel()].copy_(x.reshape(-1).to(DEV))
    view = flat[1:1 + x.numel()].view(x.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def test_self_attention_fn_on_an_unaligned_view(mode):
    """ops.SelfAttentionFn on a packed qkv one element into a flat buffer: vec_ok fails on the inputs while out, dqkv (empty_like) are
    aligned; judged like the direct launches"""
    from opentransformer_amd import ops
    name = 'sweep_d64_aligned'
    c, x = ac.build(name), ac.operands(name, mode)
    qkv = _one_off(torch.cat((x['q'], x['k'], x['v']), -1)).requires_grad_(True)
    out = ops.SelfAttentionFn.apply(qkv, c['key_mask'].to(DEV), c['H'], False)
    (g,) = torch.autograd.grad(out, qkv, x['do'].to(DEV))
    assert out.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    d, H = c['d'], c['H']
    got = {'out': out.detach(), 'dq': g[..., :d], 'dk': g[..., d:2 * d], 'dv': g[..., 2 * d:]}
    judge(name, mode, 'SelfAttentionFn unaligned', {n: ac.heads(t.cpu().double(), H) for n, t in got.items()})


def test_cross_attention_fn_on_an_unaligned_view(mode):
    """ops.CrossAttentionFn with an aligned q and the packed kv one element into a flat buffer"""
    from opentransformer_amd import ops
    name = 'cross_130x70_d64'
    c, x = ac.build(name), ac.operands(name, mode)
    q = x['q'].to(DEV).requires_grad_(True)
    kv = _one_off(torch.cat((x['k'], x['v']), -1)).requires_grad_(True)
    out = ops.CrossAttentionFn.apply(q, kv, c['key_mask'].to(DEV), c['H'])
    gq, gkv = torch.autograd.grad(out, (q, kv), x['do'].to(DEV))
    d, H = c['d'], c['H']
    got = {'out': out.detach(), 'dq': gq, 'dk': gkv[..., :d], 'dv': gkv[..., d:]}
    judge(name, mode, 'CrossAttentionFn unaligned', {n: ac.heads(t.cpu().double(), H) for n, t in got.items()})
