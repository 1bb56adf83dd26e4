"""Named cases for the GEMM core (csrc/gemm_kernel.h behind otr_linear_fwd / _dgrad / _wgrad / _fwd_batched) and the float64
reference and per-element bound they are judged by.  No GPU here: tests/test_gemm_cases.py checks on the CPU that every case is what
it claims and that the bound has teeth, tests/test_gpu_gemm.py runs the cases through the C ABI.

A case is written in the kernel's own terms, C[M,N] = act(sum_k A(m,k) B(n,k) + bias[n]) (+ C), and mapped to the entry's descriptor:
  fwd    y[M,N]  = x[M,K] w[N,K]^T      A = x  (rows x K, K contiguous: "KC")     B = w  (KC)
  dgrad  dx[M,N] = dy[M,K] w[K,N]       A = dy (KC)                               B = w  stored [K][N], rows contiguous ("MC")
  wgrad  dw[M,N] = dy[K,M]^T x[K,N]     A = dy stored [K][M] (MC)                 B = x  stored [K][N] (MC)
Operand types are 'h' (the 16-bit type of the mode; fp32 in fp32 mode) or 'f' (fp32).  K is given in the mode's units,
(full stages, tail) with tail 'CE', 'BK' or a plain count: K = full * BK + tail, BK = 64 / CE = 8 / PM = 4 in bf16 and fp16,
BK = 16 / CE = 4 / PM = 2 in fp32.  realise(name, mode) turns a case into sizes, leading dimensions and `claims`: what plan(), a Python
replay of gemm_launch_tiles, says the launcher does with it.

Bound.  a, b = the operands rounded to the compute type, c0 = the prior C of a += case, ref = a b^T + bias + c0 (then ReLU) and
S = |a| |b|^T + |bias| + |c0| in float64.  Every element must satisfy
    |got - ref| <= (K + 2) 2^-23 S + eps(out type) |ref|:
the bound of a length-K fp32 sum in any order plus one rounding to the output type (16-bit products are exact in fp32; eps is twice
the unit roundoff, which leaves a factor of two for a matrix pipe that does not round every partial sum to nearest).  floor() is a
plain fp32 emulation (BK chunks, k-slice slabs added in order, one rounding); MUTANTS are the errors the bound has to catch."""
import functools
import zlib

import torch

MODES = ('fp32', 'bf16', 'fp16')
CFG = {'fp32': dict(BK=16, CE=4, PM=2, esize=4), 'bf16': dict(BK=64, CE=8, PM=4, esize=2), 'fp16': dict(BK=64, CE=8, PM=4, esize=2)}
ENTRIES = ('fwd', 'dgrad', 'wgrad')
MODE_OF = {'fwd': ('KC', 'KC'), 'dgrad': ('KC', 'MC'), 'wgrad': ('MC', 'MC')}
RESIDENT = {64: 1024, 128: 512}               # OTR_RESIDENT_WG64 / OTR_RESIDENT_WG
WS_BYTES = 64 << 20                           # the split-K workspace the tests hand in (ops._WS_BYTES)
GUARD_ROWS = 2
FAMILIES = ('kloop', 'edges', 'epilogue', 'types', 'layout', 'splitk', 'tilemap', 'persist', 'grouped')
MUTANTS = ('last_stage', 'slab', 'bias_tail', 'frag_swap', 'tail_col')


def h16_of(mode):
    """the library's 16-bit type in this mode (fp32 mode keeps the bf16 build loaded)"""
    return torch.float16 if mode == 'fp16' else torch.bfloat16


def compute_dtype(mode):
    return torch.float32 if mode == 'fp32' else h16_of(mode)


def dtype_of(tag, mode):
    return torch.float32 if (tag == 'f' or mode == 'fp32') else h16_of(mode)


def esize(dt):
    return 4 if dt == torch.float32 else 2


# ------------------------------------------------------------------------------------------ the launcher's plan, replayed
def splits_for(tiles, nk, max_by_ws, force_ksplit):
    if max_by_ws < 2:
        return 1
    if nk <= 24 and force_ksplit == 0:
        return 1
    want = (256 + tiles // 2) // tiles if tiles >= 64 else (512 + tiles - 1) // tiles
    cap = max(nk // 4, 1)
    cap = min(cap, max_by_ws)
    return min(want, cap)


def side_fast(smode, vec, rows, K, CE, PM):
    if smode == 'KC':
        return bool(vec) and K % CE == 0 and rows > 0
    return bool(vec) and rows % PM == 0 and K % CE == 0


def side_vec(smode, off, ld, dt, PM):
    """kc_vec / mc_vec of csrc/api.hip for an operand that starts `off` elements after a 16-byte boundary"""
    es = esize(dt)
    if smode == 'KC':
        return (off * es) % 16 == 0 and ld % (16 // es) == 0
    return (off * es) % (PM * es) == 0 and ld % PM == 0


def plan(mode, entry, M, N, K, at, bt, ot, lay, accumulate=0, force_tile=0, force_ksplit=0, ws_bytes=WS_BYTES):
    """gemm_launch_tiles for one launch; at / bt / ot torch dtypes, lay = {'a' | 'b' | 'c': (off, ld)}"""
    g = CFG[mode]
    BK, CE, PM = g['BK'], g['CE'], g['PM']
    ct = compute_dtype(mode)
    nk = (K + BK - 1) // BK
    max_by_ws = ws_bytes // (M * N * 4)
    can_split = max_by_ws >= 2
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    t64 = ((M + 63) // 64) * ((N + 63) // 64)
    sf = lambda tiles: splits_for(tiles, nk, max_by_ws, force_ksplit)
    big = M >= 128 and N >= 128
    if big and t128 >= 256:
        ks = 1
    elif big and t128 * sf(t128) >= 192:
        ks = sf(t128)
    else:
        big = False
        ks = 1 if t64 >= 256 else sf(t64)
    if force_tile == 64:
        big = False
    if force_tile == 128:
        big = True
    if force_tile:
        ks = sf(t128 if big else t64)
    if force_ksplit > 0 and can_split:
        ks = min(force_ksplit, nk, max_by_ws)
    ks = max(ks, 1)
    per = (nk + ks - 1) // ks                  # every slice owns a stage
    ks = (nk + per - 1) // per
    am, bm = MODE_OF[entry]
    a_vec = side_vec(am, lay['a'][0], lay['a'][1], at, PM)
    b_vec = side_vec(bm, lay['b'][0], lay['b'][1], bt, PM)
    coff, ldc = lay['c']
    c_al = (coff * esize(ot)) % 16 == 0
    c_ok = c_al and ldc % (16 // esize(ot)) == 0 and not (accumulate and esize(ot) == 2)
    fast = side_fast(am, a_vec, M, K, CE, PM) and side_fast(bm, b_vec, N, K, CE, PM) and (ks > 1 or c_ok)
    persist = (am, bm) == ('KC', 'KC') and fast and ks == 1
    tile = 128 if big else 64
    ntiles = t128 if big else t64

    def side_depth(smode, dt):
        if not fast or dt != ct:
            return 1
        return 2 if (smode == 'KC' or esize(ct) == 2) else 1          # RAWQ / RAWT
    depth = 2 if side_depth(am, at) == 2 and side_depth(bm, bt) == 2 else 1
    passes = 0                                # generic kernels and split-K slabs store straight from the accumulators
    if fast and ks == 1:
        buf2 = 2 * (2 * tile) * (16 * (8 if esize(ct) == 2 else 4))
        crow = tile * esize(ot) + 16
        passes = 1 if tile * crow <= buf2 else 2 if tile // 2 * crow <= buf2 else 4
    reduce = 'none' if ks == 1 else ('vec4' if (N % 4 == 0 and ldc % 4 == 0 and c_al) else 'scalar')
    grid = min(ntiles, RESIDENT[tile]) if persist else ntiles
    return dict(tile=tile, ksplit=ks, per=per, nk=nk, fast=fast, persist=persist, depth=depth, passes=passes, reduce=reduce,
                ntiles=ntiles, grid=grid, rounds=(ntiles + grid - 1) // grid, t64=t64, t128=t128, swizzle=ks >= 8)


# ------------------------------------------------------------------------------------------ the cases
SPECS = {}


def _add(name, family, entry, M, N, k, at='h', bt='h', ot='h', aoff=0, boff=0, coff=0, apad=0, bpad=0, cpad=0, bias=0, relu=0, acc=0,
         tile=0, ksplit=0):
    """*pad: leading dimension = width + pad; 'chunk' = the elements of 16 bytes, 'align' = up to the next multiple of 8"""
    assert name not in SPECS, name
    assert entry == 'fwd' or not (bias or relu)               # the gradient entries have neither
    assert entry != 'wgrad' or ot == 'f'
    SPECS[name] = dict(name=name, family=family, entry=entry, M=M, N=N, k=k, at=at, bt=bt, ot=ot, aoff=aoff, boff=boff, coff=coff,
                       apad=apad, bpad=bpad, cpad=cpad, bias=bias, relu=relu, acc=acc, tile=tile, ksplit=ksplit)


def _flags(**kw):
    return ''.join('_' + k for k, v in kw.items() if v)


def _define():
    # 1. k-loop: stages 1..5 with a last stage of CE and of BK elements, at either pipeline depth, tile size and entry
    for entry in ENTRIES:
        for tile in (64, 128):
            for depth, at in ((2, 'h'), (1, 'f')):
                for s in range(1, 6):
                    for tail in ('CE', 'BK'):
                        _add('kloop_%s_t%d_d%d_s%d_%s' % (entry, tile, depth, s, tail), 'kloop', entry, 72, 80, (s - 1, tail), at=at,
                             ot='f', tile=tile)
            for full in (0, 1, 2):                             # K % CE != 0: the generic loaders
                _add('kloop_%s_t%d_generic_k%dBK3' % (entry, tile, full), 'kloop', entry, 72, 80, (full, 3), ot='f', cpad='align',
                     tile=tile)
        if entry != 'fwd':                                     # transposing loaders: row counts with % PM != 0
            for tile in (64, 128):
                _add('kloop_%s_t%d_rows71x73' % (entry, tile), 'kloop', entry, 71, 73, (2, 'CE'), ot='f', cpad='align', tile=tile)
    # 2. tile edges
    vals = (1, 15, 17, 63, 65, 127, 129)
    for i, m in enumerate(vals):
        n = vals[len(vals) - 1 - i]
        for tile in (64, 128):
            for ot in ('h', 'f'):
                for cpad in (0, 'align'):
                    _add('edges_fwd_%dx%d_t%d_%s%s' % (m, n, tile, ot, '_ldc8' if cpad else ''), 'edges', 'fwd', m, n, (1, 'CE'), ot=ot,
                         cpad=cpad, bias=1, tile=tile)
            for entry in ('dgrad', 'wgrad'):
                _add('edges_%s_%dx%d_t%d' % (entry, m, n, tile), 'edges', entry, m, n, (1, 'CE'), ot='f', tile=tile)
    for tile in (64, 128):
        for ot in ('h', 'f'):                                  # N % EPC != 0 with ldc % EPC == 0: store_tail
            _add('edges_tail_131_t%d_%s' % (tile, ot), 'edges', 'fwd', 40, 131, (1, 'CE'), ot=ot, cpad=5, bias=1, tile=tile)
        for relu in (0, 1):                                    # ... into an fp32 C +=: store_tail_acc
            _add('edges_tailacc_131_t%d%s' % (tile, _flags(relu=relu)), 'edges', 'fwd', 40, 131, (1, 'CE'), ot='f', cpad=5, bias=1,
                 relu=relu, acc=1, tile=tile)
        for acc in (0, 1):                                     # every row slab of the 2- and 4-pass staged epilogue
            _add('edges_slabs_128x72_t%d%s' % (tile, _flags(acc=acc)), 'edges', 'fwd', 128, 72, (1, 'CE'), ot='f', bias=1, acc=acc,
                 tile=tile)
    # 3. epilogue grid on the FAST and the generic kernel
    for kern, aoff in (('fast', 0), ('generic', 1)):
        for tile in (64, 128):
            for ot in ('h', 'f'):
                for bias in (0, 1):
                    for relu in (0, 1):
                        for acc in (0, 1):
                            _add('epi_%s_t%d_%s%s' % (kern, tile, ot, _flags(bias=bias, relu=relu, acc=acc)), 'epilogue', 'fwd', 72, 80,
                                 (1, 'CE'), ot=ot, aoff=aoff, bias=bias, relu=relu, acc=acc, tile=tile)
    for entry in ('dgrad', 'wgrad'):
        for ot in (('h', 'f') if entry == 'dgrad' else ('f',)):
            for acc in (0, 1):
                _add('epi_%s_%s%s' % (entry, ot, _flags(acc=acc)), 'epilogue', entry, 72, 80, (1, 'CE'), ot=ot, acc=acc, tile=64)
    # every operand / output type combination that gemm_dispatch_bf16 lists for the entry (fp32 mode: gemm_dispatch_f32 has one)
    for entry in ENTRIES:
        for at in 'hf':
            for bt in 'hf':
                for ot in ('hf' if entry != 'wgrad' else 'f'):
                    _add('types_%s_%s%s%s' % (entry, at, bt, ot), 'types', entry, 72, 80, (2, 'CE'), at=at, bt=bt, ot=ot, tile=64)
    # 4. layout: each of these takes the launch off the FAST kernel; the 'chunk' twins stay on it
    for entry in ENTRIES:
        for tag, kw in (('aoff1', dict(aoff=1)), ('boff1', dict(boff=1)), ('coff1', dict(coff=1)), ('lda1', dict(apad=1)),
                        ('ldb1', dict(bpad=1)), ('ldc1', dict(cpad=1)), ('lda_chunk', dict(apad='chunk')),
                        ('ldb_chunk', dict(bpad='chunk')), ('ldc_chunk', dict(cpad='chunk'))):
            _add('layout_%s_%s' % (entry, tag), 'layout', entry, 72, 80, (1, 'CE'), ot='f', tile=64, **kw)
    for tag, kw in (('coff1', dict(coff=1)), ('ldc1', dict(cpad=1)), ('ldc_chunk', dict(cpad='chunk'))):
        _add('layout_fwd_h_%s' % tag, 'layout', 'fwd', 72, 80, (1, 'CE'), ot='h', bias=1, tile=64, **kw)
    # 5. split-K, forced: (stages, slices asked) -> slices after "every slice owns a stage"
    for stages, asked in ((5, 4), (8, 8), (17, 16), (12, 12), (17, 17)):
        for red, n, cpad in (('vec', 80, 0), ('scalar', 131, 5), ('oddldc', 80, 1)):
            for tag, kw in (('f', dict(ot='f')), ('h_bias_relu', dict(ot='h', bias=1, relu=1)), ('f_acc', dict(ot='f', acc=1)),
                            ('h_bias_relu_acc', dict(ot='h', bias=1, relu=1, acc=1))):
                if red == 'oddldc' and tag not in ('f', 'h_bias_relu_acc'):
                    continue
                _add('splitk_s%d_a%d_%s_%s' % (stages, asked, red, tag), 'splitk', 'fwd', 136, n, (stages - 1, 'CE'), cpad=cpad, tile=64,
                     ksplit=asked, **kw)
    for stages, asked in ((8, 8), (17, 16)):                   # 3 x 2 tiles of 128; the transposing loaders under a split
        _add('splitk_s%d_a%d_t128' % (stages, asked), 'splitk', 'fwd', 264, 136, (stages - 1, 'CE'), ot='h', bias=1, tile=128, ksplit=asked)
        for entry in ('dgrad', 'wgrad'):
            _add('splitk_s%d_a%d_%s' % (stages, asked, entry), 'splitk', entry, 136, 80, (stages - 1, 'CE'), ot='f', acc=1, tile=64,
                 ksplit=asked)
    _add('splitk_unforced_97x64x2560', 'splitk', 'fwd', 97, 64, ('raw', 2560), ot='h', bias=1)      # the heuristic splits on its own
    # 6. tile map without persistence: 9 x 3 tiles, a full group of 8 row blocks and a remainder
    for tile, m, n in ((64, 8 * 64 + 17, 136), (128, 8 * 128 + 17, 264)):
        for entry in ENTRIES:
            # (wgrad: + 20 rows, its transposing A loader is FAST only with M % PM == 0)
            _add('tilemap_%s_t%d' % (entry, tile), 'tilemap', entry, m + 3 * (entry == 'wgrad'), n, (1, 'CE'), ot='f', tile=tile,
                 aoff=1 if entry == 'fwd' else 0)
        _add('tilemap_fwd_t%d_onepass' % tile, 'tilemap', 'fwd', m, n, (1, 'CE'), ot='h', bias=1, tile=tile)
    # 7. persistent walk (the only large cases): a second tile for some workgroups, a clamped and dropped re-load for the others
    for depth, at in ((2, 'h'), (1, 'f')):
        _add('persist_t64_2085x2000_d%d' % depth, 'persist', 'fwd', 2085, 2000, (2, 'CE'), at=at, ot='h', bias=1, tile=64)
        _add('persist_t128_2821x2856_d%d' % depth, 'persist', 'fwd', 2821, 2856, (2, 'CE'), at=at, ot='h', bias=1)
    # 9. the items of ONE otr_linear_wgrad_grouped call, dw[M,N] += dy[K,M]^T x[K,N] (each is a weight-gradient case of its own too):
    # eight 512 x 512 outputs over 16 rows and a ragged 200 x 136 make the 128 tiles that keep a type pair on 128-wide tiles, the
    # lone 136 x 100 of another pair falls back to 64-wide, two small ones cover the other pairs, one starts an element off
    for i in range(8):
        _add('grouped_512x512_%d' % i, 'grouped', 'wgrad', 512, 512, ('raw', 16), ot='f', acc=1)
    _add('grouped_200x136_ragged', 'grouped', 'wgrad', 200, 136, ('raw', 40), ot='f', acc=1)
    _add('grouped_136x100_lone', 'grouped', 'wgrad', 136, 100, ('raw', 24), at='f', bt='h', ot='f', acc=1)
    _add('grouped_72x52', 'grouped', 'wgrad', 72, 52, ('raw', 32), at='h', bt='f', ot='f', acc=1)
    _add('grouped_20x12', 'grouped', 'wgrad', 20, 12, ('raw', 8), at='f', bt='f', ot='f', acc=1)
    _add('grouped_72x52_off1', 'grouped', 'wgrad', 72, 52, ('raw', 32), ot='f', aoff=1, acc=1)


_define()
NAMES = tuple(SPECS)
BIG = tuple(n for n in NAMES if SPECS[n]['family'] == 'persist')


def _pad(p, dt):
    return 16 // esize(dt) if p == 'chunk' else p


def realise(name, mode):
    """the case in one mode: sizes, types, leading dimensions and the launcher's plan for them (`claims`)"""
    s = SPECS[name]
    g = CFG[mode]
    full, tail = s['k']
    K = tail if full == 'raw' else full * g['BK'] + (g[tail] if isinstance(tail, str) else tail)
    M, N, entry = s['M'], s['N'], s['entry']
    at, bt, ot = (dtype_of(s[x], mode) for x in ('at', 'bt', 'ot'))
    am, bm = MODE_OF[entry]
    shape = {'a': (M, K) if am == 'KC' else (K, M), 'b': (N, K) if bm == 'KC' else (K, N), 'c': (M, N)}   # as stored: rows x width
    lay = {}
    for x, dt in (('a', at), ('b', bt), ('c', ot)):
        w, p = shape[x][1], s[x + 'pad']
        lay[x] = (s[x + 'off'], (w + 7) // 8 * 8 if p == 'align' else w + _pad(p, dt))
    c = dict(s, mode=mode, K=K, at=at, bt=bt, ot=ot, shape=shape, lay=lay)
    c['claims'] = plan(mode, entry, M, N, K, at, bt, ot, lay, s['acc'], s['tile'], s['ksplit'])
    c['key'] = (entry, M, N, K, at, bt, ot, tuple(sorted(lay.items())), s['bias'], s['relu'], s['acc'], s['tile'], s['ksplit'])
    return c


@functools.lru_cache(maxsize=None)
def names_for(mode):
    """the cases of a mode without the ones that fall together there (fp32 has one operand type and one depth per entry)"""
    seen, out = set(), []
    for n in NAMES:
        k = realise(n, mode)['key']
        if k not in seen:
            seen.add(k)
            out.append(n)
    return tuple(out)


def descriptor(c):
    """(M, N, K, x, w, y types, ldx, ldw, ldy) of otr_linear_desc_t and which of a / b / c is x, w, y"""
    M, N, K, lay = c['M'], c['N'], c['K'], c['lay']
    if c['entry'] == 'fwd':
        role = dict(x='a', w='b', y='c')
        dims = (M, N, K)
    elif c['entry'] == 'dgrad':                                # dx[M, Kd] = dy[M, Nd] w[Nd, Kd]: Kd = N, Nd = K
        role = dict(y='a', w='b', x='c')
        dims = (M, K, N)
    else:                                                      # dw[Nd, Kd] = dy[Md, Nd]^T x[Md, Kd]: Nd = M, Kd = N, Md = K
        role = dict(y='a', x='b', w='c')
        dims = (K, M, N)
    return dims, role, {r: lay[o][1] for r, o in role.items()}


def grouped_plan(mode):
    """{name: 64 | 128 | 'standalone'}: how otr_linear_wgrad_grouped (csrc/api.hip, the 256-wide launch switched off) serves the
    items of the 'grouped' family handed to it in one call"""
    g = CFG[mode]
    cs = [realise(n, mode) for n in NAMES if SPECS[n]['family'] == 'grouped']
    out, t128 = {}, {}
    for c in cs:
        (aoff, lda), (boff, ldb), (coff, ldc) = c['lay']['a'], c['lay']['b'], c['lay']['c']
        fast = side_vec('MC', aoff, lda, c['at'], g['PM']) and side_vec('MC', boff, ldb, c['bt'], g['PM']) and \
            c['M'] % g['PM'] == 0 and c['N'] % g['PM'] == 0 and c['K'] % (8 if mode != 'fp32' else 4) == 0 and \
            (coff * 4) % 16 == 0 and ldc % 4 == 0
        key = (c['at'], c['bt'])
        out[c['name']] = 'standalone' if not fast else (128, key) if (c['M'] >= 128 and c['N'] >= 96) else 64
        if fast and out[c['name']] != 64:
            t128[key] = t128.get(key, 0) + ((c['M'] + 127) // 128) * ((c['N'] + 127) // 128)
    return {n: (v if not isinstance(v, tuple) else 128 if t128[v[1]] >= 128 else 64) for n, v in out.items()}


# ------------------------------------------------------------------------------------------ operands, reference, bound
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)


def operands(c):
    """A [M,K], B [N,K] in their storage types (GEMM orientation; storage() transposes the MC ones), bias f32 [N] with every
    |bias| >= 0.5 (a dropped bias must show on a single element), c0 [M,N] in the output type"""
    g = _gen(c['name'])
    M, N, K = c['M'], c['N'], c['K']
    A = torch.randn(M, K, generator=g).to(c['at'])
    B = torch.randn(N, K, generator=g).to(c['bt'])
    r = torch.randn(N, generator=g)
    bias = (torch.sign(r) + (r == 0).float()) * (0.5 + r.abs()) if c['bias'] else None
    c0 = torch.randn(M, N, generator=g).to(c['ot']) if c['acc'] else None
    return A, B, bias, c0


def storage(c, x, t):
    am, bm = MODE_OF[c['entry']]
    return t.t().contiguous() if (x == 'a' and am == 'MC') or (x == 'b' and bm == 'MC') else t


def reference(c, ops=None, device='cpu'):
    """float64: (ref, S, pre) with pre = ref before the ReLU"""
    A, B, bias, c0 = ops or operands(c)
    ct = compute_dtype(c['mode'])
    a, b = A.to(device).to(ct).double(), B.to(device).to(ct).double()
    pre, S = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        pre, S = pre + bias.to(device).double(), S + bias.to(device).double().abs()
    if c0 is not None:
        pre, S = pre + c0.to(device).double(), S + c0.to(device).double().abs()
    return (pre.clamp_min(0) if c['relu'] else pre), S, pre


def bound(c, ref, S):
    return (c['K'] + 2) * 2.0 ** -23 * S + float(torch.finfo(c['ot']).eps) * ref.abs()


def slices(c):
    """[k0, k1) of every k-slice of the claimed plan"""
    cl, BK = c['claims'], CFG[c['mode']]['BK']
    return [(s * cl['per'] * BK, min((s + 1) * cl['per'] * BK, c['K'])) for s in range(cl['ksplit'])]


def floor(c, ops=None):
    """the result in a plain emulation of the working precision: fp32 sums over BK chunks, the slabs of the k-slices added in
    order, bias, prior C, ReLU, one rounding to the output type"""
    A, B, bias, c0 = ops or operands(c)
    ct, BK = compute_dtype(c['mode']), CFG[c['mode']]['BK']
    a, b = A.to(ct).float(), B.to(ct).float()
    total = None
    for k0, k1 in slices(c):
        slab = torch.zeros(c['M'], c['N'])
        for k in range(k0, k1, BK):
            slab = slab + a[:, k:min(k + BK, k1)] @ b[:, k:min(k + BK, k1)].t()
        total = slab if total is None else total + slab
    if bias is not None:
        total = total + bias
    if c0 is not None:
        total = total + c0.float()
    if c['relu']:
        total = total.clamp_min(0)
    return total.to(c['ot'])


def violations(c, got, ref, S):
    """elements outside the bound (a NaN is outside it), float64 [M, N] -> bool"""
    return ~((got.double() - ref).abs() <= bound(c, ref, S))


def worst(c, got, ref, S):
    """the worst ratio error / bound and where it is, for the report of a failure"""
    ratio = (got.double() - ref).abs() / bound(c, ref, S).clamp_min(1e-300)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    i = int(ratio.argmax())
    r, col = i // c['N'], i % c['N']
    return dict(ratio=float(ratio.reshape(-1)[i]), row=r, col=col, got=float(got.reshape(-1)[i]), ref=float(ref.reshape(-1)[i]),
                tile64=(r // 64, col // 64), tile128=(r // 128, col // 128), bad=int((ratio > 1).sum()))


def mutant(c, kind, ops=None, refs=None):
    """(result, region): the expected result with one of the errors the suite exists to catch, and the elements it touches;
    None where the case has nothing of that kind"""
    A, B, bias, c0 = ops or operands(c)
    ref, S, pre = refs or reference(c, (A, B, bias, c0))
    ct, g = compute_dtype(c['mode']), CFG[c['mode']]
    M, N, K = c['M'], c['N'], c['K']
    act = (lambda t: t.clamp_min(0)) if c['relu'] else (lambda t: t)
    region = torch.zeros(M, N, dtype=torch.bool)

    def without_k(k0, k1):
        a, b = A[:, k0:k1].to(ct).double(), B[:, k0:k1].to(ct).double()
        return act(pre - a @ b.t())
    if kind == 'last_stage':                                   # the last (partial) k-stage never multiplied
        region[:] = True
        return without_k((c['claims']['nk'] - 1) * g['BK'], K), region
    if kind == 'slab':                                         # one k-slice's slab left out of the reduce
        if c['claims']['ksplit'] < 2:
            return None
        region[:] = True
        return without_k(*slices(c)[1]), region
    if kind == 'bias_tail':                                    # no bias on the last (partial) 16-byte chunk of a row
        if bias is None:
            return None
        epc = 16 // esize(c['ot'])
        n0 = N - (N % epc or min(epc, N))
        out = pre.clone()
        out[:, n0:] -= bias[n0:].double()
        region[:, n0:] = True
        return act(out), region
    if kind == 'frag_swap':                                    # two 4-column groups of one 16 x 16 fragment exchanged
        if N < 8:
            return None
        r0, c0_ = 16 * ((M - 1) // 16), 16 * ((N - 8) // 16)
        out = ref.clone()
        out[r0:r0 + 16, c0_:c0_ + 4] = ref[r0:r0 + 16, c0_ + 4:c0_ + 8]
        out[r0:r0 + 16, c0_ + 4:c0_ + 8] = ref[r0:r0 + 16, c0_:c0_ + 4]
        region[r0:r0 + 16, c0_:c0_ + 8] = True
        return out, region
    if kind == 'tail_col':                                     # the last column keeps what C held before
        out = ref.clone()
        out[:, N - 1] = c0[:, N - 1].double() if c0 is not None else float('nan')
        region[:, N - 1] = True
        return out, region
    raise KeyError(kind)
