"""GPU (-m gpu): the GEMM core (csrc/gemm_kernel.h) through otr_linear_fwd / _dgrad / _wgrad / _fwd_batched, per output element.

Every case of tests/gemm_cases.py (checked on the CPU by tests/test_gemm_cases.py) runs in fp32, bf16 and fp16 on (pointer, leading
dimension) operands that live inside larger buffers: the columns between the logical width and the leading dimension, two guard rows
before and after and the row between two batches hold NaN.  After the call
  - every element of C satisfies |got - ref| <= (K + 2) 2^-23 S + eps(out) |ref| against float64 (gemm_cases.bound; no norm anywhere),
  - no element of C is NaN (a clamped or unconditional load must be discarded by a select, never by a multiply with zero),
  - everything outside the logical C has the bits it had before,
  - the otr_debug_trace stamps -- four per (k-slice, tile) at ((kslice * ntiles + tile) * 4) -- show exactly ntiles * ksplit groups
    for the tile size and slice count that gemm_cases.plan() claims (the shapes have different 64- and 128-wide tile counts wherever
    they are large enough to).
otr_linear_wgrad_grouped gets the items of the 'grouped' family, an M = 0 item among them, in ONE call with key 6 = 0 (the 256-wide
launch of csrc/wgrad256.hip, which has tests of its own, takes nothing).
A failure names the worst element with its row and column tile at either tile size.  The debug keys 0 (tile), 1 (split-K) and 6 and the
trace pointer are back at their defaults after every test.  Every test adds the worst error / bound ratio it saw to
parity_out/gemm_parity.json (or under $OTR_PARITY_DIR), per mode and family, before it asserts.

Measured on MI355X, worst error / bound over every case of a mode: bf16 0.50, fp16 0.49 (the one rounding to a 16-bit output, unit
roundoff over eps; 0.10 / 0.17 over the fp32-output families), fp32 0.19 (kloop_*_generic_k0BK3: K = 3).  The bound was not fitted
to these: it is the derivation in tests/gemm_cases.py.
Six mutations of csrc/gemm_kernel.h were run against this module (bf16 and fp32; none reads or writes out of bounds), each fails it:
no k-tail mask in the raw row-major FAST store (241 cases: every FAST forward case whose last stage is partial, all of split-K);
store_tail_acc without its ReLU (the four edges_tailacc_131_*_relu); gemm_tile_of's remainder row blocks starting at 0 (tilemap_*
and persist_t128_*: the last row block keeps its NaN); the reduce's remainder loop one slab short (splitk_s12_a12_vec_* and
splitk_unforced_*); the row slabs of the multi-pass staged epilogue all written to the first slab's rows (190 cases: every FAST
fp32 case, every fp32-output case on 128-wide tiles); two 4-column groups of one fragment exchanged on their way to the staging
LDS (299 cases)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_WS = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


def _report(c, family, ratio):
    key = '%s/%s' % (c['mode'], family)
    rec = REPORT.setdefault(key, {'cases': 0, 'worst': 0.0, 'at': ''})
    rec['cases'] += 1
    if not ratio <= rec['worst']:
        rec['worst'], rec['at'] = float('%.3g' % ratio), c['name']
    out = os.environ.get('OTR_PARITY_DIR') or os.path.join(ROOT, 'parity_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'gemm_parity.json'), 'w') as f:
        json.dump(REPORT, f, sort_keys=True, indent=None, separators=(',', ':'))


def _lib(mode):
    from opentransformer_amd import ops, _lib as L
    ops.set_compute_dtype(mode)
    return L.load(), L, ops._compute_code()


@pytest.fixture
def knobs():
    """otr_debug_set / otr_debug_trace for one test; keys 0, 1 and 6 and the trace pointer return to their defaults whatever happens"""
    from opentransformer_amd import ops, _lib as L
    libs = []

    def use(lib, tile=0, ksplit=0, wgrad256=-1):
        libs.append(lib)
        assert lib.otr_debug_set(0, tile) == 0 and lib.otr_debug_set(1, ksplit) == 0 and lib.otr_debug_set(6, wgrad256) == 0
    try:
        yield use
    finally:
        for lib in libs:
            lib.otr_debug_set(0, 0)
            lib.otr_debug_set(1, 0)
            lib.otr_debug_set(6, -1)                           # -1: the environment decides again, as at start-up
            lib.otr_debug_trace(None)
        ops.set_compute_dtype('bf16')


def _workspace():
    if 'ws' not in _WS:
        _WS['ws'] = torch.empty(gc.WS_BYTES // 4, dtype=torch.float32, device=DEV)
    return _WS['ws']


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """nb matrices [rows, width] with leading dimension ld, one NaN row between two of them, starting `off` elements after a
    16-byte boundary behind two guard rows; everything that is not an element of a matrix holds NaN"""

    def __init__(self, rows, width, off, ld, dtype, value=None, nb=1):
        assert ld >= width and off >= 0
        self.rows, self.width, self.ld, self.nb, self.dtype = rows, width, ld, nb, dtype
        self.lead = (gc.GUARD_ROWS * ld + 15) // 16 * 16 + off
        self.bs = (rows + 1) * ld                              # elements from one batch to the next
        n = self.lead + nb * self.bs + gc.GUARD_ROWS * ld + 16
        host = torch.full((n,), NAN, dtype=dtype)
        own = torch.zeros(n, dtype=torch.bool)
        size, stride = (nb, rows, width), (self.bs, ld, 1)
        own.as_strided(size, stride, self.lead).fill_(True)
        if value is not None:
            host.as_strided(size, stride, self.lead).copy_(value.reshape(size))
        self.buf = host.to(DEV)
        self.own = own.to(DEV)
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0
        assert self.lead + (nb - 1) * self.bs + (rows - 1) * ld + width <= n - gc.GUARD_ROWS * ld          # the guards stay guards

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.lead * self.buf.element_size())

    def logical(self):
        t = self.buf.as_strided((self.nb, self.rows, self.width), (self.bs, self.ld, 1), self.lead)
        return t[0] if self.nb == 1 else t

    def outside_unchanged(self):
        b = BITS[self.dtype]
        return torch.equal(self.buf.view(b)[~self.own], self.before.view(b)[~self.own])

    def untouched(self):
        b = BITS[self.dtype]
        return torch.equal(self.buf.view(b), self.before.view(b))


def _buffers(c, ops, nb=1):
    A, B, bias, c0 = ops
    ga = Guarded(*c['shape']['a'], *c['lay']['a'], c['at'], gc.storage(c, 'a', A) if nb == 1 else A, nb)
    gb = Guarded(*c['shape']['b'], *c['lay']['b'], c['bt'], gc.storage(c, 'b', B) if nb == 1 else B, nb)
    gcc = Guarded(*c['shape']['c'], *c['lay']['c'], c['ot'], c0, nb)
    return ga, gb, gcc, (bias.to(DEV) if bias is not None else None)


def _descriptor(c, L, compute, types=None):
    (Md, Nd, Kd), role, ld = gc.descriptor(c)
    code = {torch.float32: L.OTR_F32, torch.bfloat16: L.OTR_BF16, torch.float16: L.OTR_F16}
    t = types or {'a': c['at'], 'b': c['bt'], 'c': c['ot']}
    return L.LinearDesc(Md, Nd, Kd, code[t[role['x']]], code[t[role['w']]], code[t[role['y']]], compute, ld['x'], ld['w'], ld['y'],
                        L.ACT_RELU if c['relu'] else L.ACT_NONE, c['acc'])


def _call(c, lib, d, ga, gb, gcc, bias):
    ws = _workspace()
    wsp, wsb = C.c_void_p(ws.data_ptr()), gc.WS_BYTES
    if c['entry'] == 'fwd':
        return lib.otr_linear_fwd(C.byref(d), ga.ptr(), gb.ptr(), C.c_void_p(bias.data_ptr()) if bias is not None else None, gcc.ptr(),
                                  wsp, wsb, _stream())
    if c['entry'] == 'dgrad':
        return lib.otr_linear_dgrad(C.byref(d), ga.ptr(), gb.ptr(), gcc.ptr(), wsp, wsb, _stream())
    return lib.otr_linear_wgrad(C.byref(d), ga.ptr(), gb.ptr(), gcc.ptr(), wsp, wsb, _stream())


def _judge(c, got, ref, S, what='', family=None):
    ratio = ((got.to(ref.device).double() - ref).abs() / gc.bound(c, ref, S).clamp_min(1e-300)).max()
    _report(c, family or c.get('family', 'batched'), float('inf') if bool(torch.isnan(ratio)) else float(ratio))
    assert not bool(torch.isnan(got).any()), '%s %s: %d NaN in the output, first at %s' % (
        c['name'], what, int(torch.isnan(got).sum()), torch.isnan(got).nonzero()[0].tolist())
    bad = gc.violations(c, got.to(ref.device), ref, S)
    if bool(bad.any()):
        if got.dim() == 3:                                     # batched: report the worst batch
            z = int(bad.flatten(1).sum(1).argmax())
            w = dict(gc.worst(c, got[z].to(ref.device), ref[z], S[z]), batch=z)
        else:
            w = gc.worst(c, got.to(ref.device), ref, S)
        pytest.fail('%s %s: %d elements outside the bound; worst %r; plan %r' % (c['name'], what, int(bad.sum()), w, c.get('claims')))


def _stamps(trace, c):
    """(number of stamped groups, they are the first ones, every group has its four stamps, largest stamped k-slice)"""
    cl = c['claims']
    g = trace.view(-1, 4).cpu() != 0
    hit = g.any(1)
    n = int(hit.sum())
    idx = hit.nonzero().flatten()
    return n, bool(hit[:n].all()), bool(g[hit].all()), (int(idx.max()) // cl['ntiles'] if n else -1)


# ------------------------------------------------------------------------------------------ fwd / dgrad / wgrad
def _run_case(mode, name, knobs):
    lib, L, compute = _lib(mode)
    c = gc.realise(name, mode)
    cl = c['claims']
    ops = gc.operands(c)
    dev = DEV if name in gc.BIG else 'cpu'                     # the two large shapes: float64 on the device
    ref, S, _ = gc.reference(c, ops, device=dev)
    ga, gb, gcc, bias = _buffers(c, ops)
    d = _descriptor(c, L, compute)
    # stamps land at ((kslice * ntiles + tile) * 4 + slot) with kslice < ksplit <= nk and tile < ntiles <= t64: room for any plan
    trace = torch.zeros(cl['t64'] * cl['nk'] * 4, dtype=torch.int64, device=DEV)
    if cl['ksplit'] > 1:                                       # a slab element that no slice writes must show
        _workspace()[:c['M'] * c['N'] * cl['nk']].fill_(NAN)
    knobs(lib, c['tile'], c['ksplit'])
    torch.cuda.synchronize()
    try:
        lib.otr_debug_trace(C.c_void_p(trace.data_ptr()))
        rc = _call(c, lib, d, ga, gb, gcc, bias)
        torch.cuda.synchronize()
    finally:
        lib.otr_debug_trace(None)
    assert rc == 0, (rc, lib.otr_last_error_string())
    n, first, whole, top = _stamps(trace, c)
    assert (n, first, whole, top) == (cl['ntiles'] * cl['ksplit'], True, True, cl['ksplit'] - 1), \
        '%s: %d stamped groups, largest slice %d; the plan %r has %d tiles x %d slices (64-wide %d, 128-wide %d tiles)' % (
            name, n, top, cl, cl['ntiles'], cl['ksplit'], cl['t64'], cl['t128'])
    _judge(c, gcc.logical(), ref, S)
    assert gcc.outside_unchanged(), '%s: C changed outside [0:M, 0:N]' % name
    assert ga.untouched() and gb.untouched()


def _ids(pairs):
    return ['%s-%s' % p for p in pairs]


CASES = [(m, n) for m in gc.MODES for n in gc.names_for(m)]


@pytest.mark.parametrize('mode,name', CASES, ids=_ids(CASES))
def test_gemm_case(mode, name, knobs):
    _run_case(mode, name, knobs)


@pytest.mark.parametrize('mode', gc.MODES)
def test_unlisted_type_combination_is_refused(mode, knobs):
    """gemm_dispatch_bf16 lists no weight gradient into a 16-bit dw, gemm_dispatch_f32 nothing but fp32: refused, nothing written"""
    lib, L, compute = _lib(mode)
    knobs(lib)
    name = 'epi_wgrad_f' if mode != 'fp32' else 'epi_fast_t64_f'
    c = gc.realise(name, mode)
    h = gc.h16_of(mode)
    types = {'a': c['at'], 'b': c['bt'], 'c': h} if mode != 'fp32' else {'a': h, 'b': c['bt'], 'c': c['ot']}
    ga, gb, gcc, bias = _buffers(c, gc.operands(c))             # (the buffers keep the sizes of the wider type)
    rc = _call(c, lib, _descriptor(c, L, compute, types), ga, gb, gcc, bias)
    torch.cuda.synchronize()
    assert rc < 0, rc
    assert gcc.untouched() and ga.untouched() and gb.untouched()


# ------------------------------------------------------------------------------------------ otr_linear_fwd_batched
# (name, M, N, K, nbatch, x / w / y types): the three type sets the kernel is built for; 64-wide tiles unless M >= 128, N >= 96 and
# 128-wide tiles x nbatch >= 240
BATCHED = (('nb2_hhf', 70, 50, 128, 2, 'h', 'h', 'f'), ('nb2_hhh', 70, 50, 128, 2, 'h', 'h', 'h'), ('nb2_fhh', 70, 50, 128, 2, 'f', 'h', 'h'),
           ('nb5_hhf', 65, 129, 136, 5, 'h', 'h', 'f'), ('nb5_hhh', 65, 129, 136, 5, 'h', 'h', 'h'), ('nb5_fhh', 65, 129, 136, 5, 'f', 'h', 'h'),
           ('nb120_t128_hhh', 256, 128, 128, 120, 'h', 'h', 'h'), ('nb120_t128_ragged_hhf', 250, 120, 128, 120, 'h', 'h', 'f'),
           ('nb120_t128_ragged_fhh', 250, 120, 128, 120, 'f', 'h', 'h'))


def _batched_case(mode, M, N, K, nb, xt, wt, yt, name='batched', ldk=None, coff=0):
    ldk = ldk or K
    ldc = (N + 7) // 8 * 8
    c = dict(name='batched_' + name, mode=mode, entry='fwd', M=M, N=N, K=K, at=gc.dtype_of(xt, mode), bt=gc.dtype_of(wt, mode),
             ot=gc.dtype_of(yt, mode), bias=0, relu=0, acc=0, shape={'a': (M, K), 'b': (N, K), 'c': (M, N)},
             lay={'a': (0, ldk), 'b': (0, ldk), 'c': (coff, ldc)})
    g = gc._gen(c['name'])
    A = torch.randn(nb, M, K, generator=g).to(c['at'])
    B = torch.randn(nb, N, K, generator=g).to(c['bt'])
    return c, (A, B, None, None)


def _batched_call(c, lib, L, compute, ga, gb, gcc, nb):
    d = _descriptor(c, L, compute)
    return lib.otr_linear_fwd_batched(C.byref(d), ga.ptr(), gb.ptr(), gcc.ptr(), nb, ga.bs, gb.bs, gcc.bs, _stream())


@pytest.mark.parametrize('mode', ('bf16', 'fp16'))
@pytest.mark.parametrize('spec', BATCHED, ids=[s[0] for s in BATCHED])
def test_batched(mode, spec, knobs):
    name, M, N, K, nb, xt, wt, yt = spec
    lib, L, compute = _lib(mode)
    knobs(lib)
    c, ops = _batched_case(mode, M, N, K, nb, xt, wt, yt, name)
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    assert (M >= 128 and N >= 96 and t128 * nb >= 240) == ('t128' in name)
    ga, gb, gcc, _ = _buffers(c, ops, nb)
    for g in (ga, gb, gcc):                                    # byte strides the kernel accepts, and batches that overlap nothing
        assert (g.bs * g.buf.element_size()) % 16 == 0 and g.bs >= g.rows * g.ld
    rc = _batched_call(c, lib, L, compute, ga, gb, gcc, nb)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.otr_last_error_string())
    ct = gc.compute_dtype(mode)
    a, b = ops[0].to(ct).double(), ops[1].to(ct).double()
    ref, S = a @ b.transpose(1, 2), a.abs() @ b.abs().transpose(1, 2)
    _judge(c, gcc.logical(), ref, S)
    assert gcc.outside_unchanged(), '%s: C changed outside the batches' % name
    assert ga.untouched() and gb.untouched()


@pytest.mark.parametrize('form', ('k_not_chunks', 'c_unaligned', 'fp32_compute', 'one_batch'))
def test_batched_refuses_what_it_is_not_built_for(form, knobs):
    """not served = 1, nothing written: the caller then loops over otr_linear_fwd"""
    mode = 'fp32' if form == 'fp32_compute' else 'bf16'
    lib, L, compute = _lib(mode)
    knobs(lib)
    kw = {'k_not_chunks': dict(K=132, ldk=136), 'c_unaligned': dict(K=128, coff=1)}.get(form, dict(K=128))
    nb = 1 if form == 'one_batch' else 3
    c, ops = _batched_case(mode, 70, 48, kw.pop('K'), nb, 'h', 'h', 'h', form, **kw)
    ga, gb, gcc, _ = _buffers(c, ops, nb)
    rc = _batched_call(c, lib, L, compute, ga, gb, gcc, nb)
    torch.cuda.synchronize()
    assert rc == 1, (rc, lib.otr_last_error_string())
    assert gcc.untouched() and ga.untouched() and gb.untouched()


# ------------------------------------------------------------------------------------------ otr_linear_wgrad_grouped
@pytest.mark.parametrize('mode', gc.MODES)
def test_grouped_wgrad_one_call(mode, knobs):
    lib, L, compute = _lib(mode)
    knobs(lib, wgrad256=0)
    gp = gc.grouped_plan(mode)
    code = {torch.float32: L.OTR_F32, torch.bfloat16: L.OTR_BF16, torch.float16: L.OTR_F16}
    cases, bufs, refs = [], [], []
    for name in gp:
        c = gc.realise(name, mode)
        ops = gc.operands(c)
        cases.append(c)
        refs.append(gc.reference(c, ops))
        bufs.append(_buffers(c, ops))
    z = gc.realise('grouped_20x12', mode)                      # the same shape again with M = 0: nothing to add, dw stays as it is
    zbuf = _buffers(z, gc.operands(z))
    items = (L.WgradItem * (len(cases) + 1))()
    order = list(range(len(cases)))
    order.insert(3, None)                                      # the empty item in the middle of the call
    for it, i in zip(items, order):
        c, (ga, gb, gcc, _) = (cases[i], bufs[i]) if i is not None else (z, zbuf)
        it.dy, it.x, it.dw = ga.ptr().value, gb.ptr().value, gcc.ptr().value
        it.M, it.N, it.K = (c['K'] if i is not None else 0), c['M'], c['N']
        it.ldy, it.ldx, it.ldw = c['lay']['a'][1], c['lay']['b'][1], c['lay']['c'][1]
        it.dy_dtype, it.x_dtype, it.dbias, it.overwrite = code[c['at']], code[c['bt']], None, 0
    ws = _workspace()
    rc = lib.otr_linear_wgrad_grouped(items, len(items), compute, C.c_void_p(ws.data_ptr()), gc.WS_BYTES, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.otr_last_error_string())
    assert all(g.untouched() for g in zbuf[:3]), 'the M = 0 item was touched'
    for c, (ga, gb, gcc, _), (ref, S, _p) in zip(cases, bufs, refs):
        _judge(c, gcc.logical(), ref, S, what='(grouped call: %r)' % (gp[c['name']],), family='grouped_call')
        assert gcc.outside_unchanged(), '%s: dw changed outside [0:N, 0:K]' % c['name']
        assert ga.untouched() and gb.untouched()
