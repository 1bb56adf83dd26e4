"""Named cases for the CTC loss kernel (csrc/ctc.hip) and the float64 reference they are judged by.  No GPU here:
tests/test_ctc_loss_cases.py checks on the CPU that every case is what its name says, tests/test_gpu_ctc_loss.py runs them.

The kernel puts one thread on each extended-label state s (0 = blank, 2i + 1 = label i, S = 2L + 1 <= 256), so states 64, 128
and 192 open the second, third and fourth wavefront of the workgroup.  The cases put the last live state on either side of
each of those boundaries, a repeated label pair across them, and the degenerate ends (one alignment, none, no labels, no frames).

reference() is F.log_softmax + F.ctc_loss ('mean', zero_infinity=True) in float64 on the CPU, the call model/ctc.py of the
reference project makes; floor() is the same call in float32 and its per-utterance distance from float64, the noise a log-space
fp32 recursion is entitled to."""
import functools

import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)
WAVE_LENGTHS = [31, 32, 33, 63, 64, 65, 95, 96, 127]      # last live state 62 | 64 | 66, 126 | 128 | 130, 190 | 192, 254
STRADDLE_AT = [31, 63, 95]                                # labels i, i + 1 sit on states 2i + 1, 2i + 3: 63 | 65, 127 | 129, 191 | 193


# ------------------------------------------------------------------------------------------ reference
def effective_lengths(targets, in_len, tgt_len, T):
    """What the kernel documents for lengths F.ctc_loss refuses: in_len is clamped to [0, T]; a target length outside
    [0, padded width] is never computed and scores like an utterance without frames or labels (nll 0, no gradient, and a
    divisor max(L, 1) = 1 that adds nothing to the mean).  Returns (in_len, tgt_len, guarded[B] bool)."""
    W = targets.shape[1]
    tl = tgt_len.long()
    guarded = (tl < 0) | (tl > W)
    il = in_len.long().clamp(0, T)
    return torch.where(guarded, torch.zeros_like(il), il), torch.where(guarded, torch.zeros_like(tl), tl), guarded


def _ctc(logits, targets, in_len, tgt_len, blank, dtype):
    B, T, V = logits.shape
    il, tl, _ = effective_lengths(targets, in_len, tgt_len, T)
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    lp = F.log_softmax(x, -1).transpose(0, 1)
    tg = targets.cpu().long()
    loss = F.ctc_loss(lp, tg, il, tl, blank=blank, reduction='mean', zero_infinity=True)
    (g,) = torch.autograd.grad(loss, x)
    with torch.no_grad():
        nll = F.ctc_loss(lp, tg, il, tl, blank=blank, reduction='none', zero_infinity=True)
    return loss.detach(), nll.detach(), g


def reference(logits, targets, in_len, tgt_len, blank):
    """float64 (loss, nll[B], dlogits[B, T, V]); nll of an infeasible utterance is 0 (zero_infinity)"""
    return _ctc(logits, targets, in_len, tgt_len, blank, torch.float64)


def nll_rel(a, ref):
    """|a - ref| / |ref| per utterance (float64); where ref is 0 (infeasible: exact zero expected) the absolute difference"""
    a, ref = a.double().cpu(), ref.double()
    d = (a - ref).abs()
    return torch.where(ref != 0, d / ref.abs().clamp_min(1e-300), d)


def slab_rel(a, ref):
    """relative Frobenius distance of each utterance's [T, V] gradient slab (float64); a zero reference slab gives the norm of a"""
    a, ref = a.double().cpu(), ref.double()
    d = (a - ref).flatten(1).norm(dim=1)
    n = ref.flatten(1).norm(dim=1)
    return torch.where(n > 0, d / n.clamp_min(1e-300), d)


def coef(tgt_len, targets, B):
    """d loss / d nll_b = 1 / (B * max(L_b, 1)) per utterance (float64); guarded utterances count with L = 0"""
    tl = tgt_len.long()
    tl = torch.where((tl < 0) | (tl > targets.shape[1]), torch.zeros_like(tl), tl)
    return 1.0 / (B * tl.clamp_min(1).double())


def rowsum_rel(g, in_len, cf):
    """per utterance, worst over the frames t < in_len_b of |sum_v g[b, t, :]| / coef_b: coef * (1 - sum_s gamma_t(s)), zero in
    exact arithmetic.  The sum itself is taken in float64."""
    g = g.double().cpu()
    B, T, _ = g.shape
    rs = g.sum(-1).abs()
    live = torch.arange(T)[None, :] < in_len.long().clamp(0, T)[:, None]
    return (rs * live).max(dim=1).values / cf


def floor(logits, targets, in_len, tgt_len, blank, ref=None):
    """The same call in float32 on the CPU and its distance from float64, per utterance: {'loss': |loss32 - loss64| / |loss64|,
    'nll': nll_rel, 'grad': slab_rel, 'rowsum': rowsum_rel of the float32 gradient}."""
    loss64, nll64, g64 = ref if ref is not None else reference(logits, targets, in_len, tgt_len, blank)
    loss32, nll32, g32 = _ctc(logits, targets, in_len, tgt_len, blank, torch.float32)
    B, T, _ = logits.shape
    il, _, _ = effective_lengths(targets, in_len, tgt_len, T)
    return {'loss': float((loss32.double() - loss64).abs() / loss64.abs().clamp_min(1e-300)), 'nll': nll_rel(nll32, nll64),
            'grad': slab_rel(g32, g64), 'rowsum': rowsum_rel(g32, il, coef(tgt_len, targets, B))}


def tiny(logits, in_len):
    """Slack for utterances whose float32 floor is (nearly) zero, per utterance: delta_b = T_b * eps_fp32 * max |lp_b|.

    alpha_t(s) + beta_t(s) - lp - ll, the exponent of every occupancy, is a sum of about T_b log-probabilities, each at most
    max |lp_b| in magnitude (taken over the frames t < T_b in float64), every one carrying a rounding of at most eps_fp32
    relative: delta_b bounds the absolute error of such a sum to first order with every rounding counted once.  It is an
    absolute error of nll_b, and since exp(delta) - 1 = delta a relative error of the occupancies, hence of the gradient slab
    and, over coef_b, of a frame's column sum.  Where one alignment exists or L = 0 the float32 reference can be exact by
    construction (floor 0) while expf / logf on the device round: that is what this term is for."""
    lp = F.log_softmax(logits.detach().cpu().double(), -1)
    B, T, _ = lp.shape
    il = in_len.long().clamp(0, T)
    live = (torch.arange(T)[None, :] < il[:, None])[:, :, None]
    m = (lp.abs() * live).flatten(1).max(dim=1).values
    return il.double() * EPS32 * m


# ------------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _labels(g, L, V, blank, distinct_neighbours=False):
    """L labels from the V - 1 symbols that are not `blank`; with distinct_neighbours no two adjacent labels are equal"""
    r = torch.randint(0, V - 1, (L,), generator=g)
    if distinct_neighbours:
        for i in range(1, L):
            while int(r[i]) == int(r[i - 1]):
                r[i] = int(torch.randint(0, V - 1, (1,), generator=g))
    return torch.where(r >= blank, r + 1, r)


def _pad(rows, width=None, blank=0, V=2):
    """[B, width] int64; the padding is an in-range label that is not the blank (never read: positions >= tgt_len)"""
    width = max([len(r) for r in rows] + [1]) if width is None else width
    out = torch.full((len(rows), width), 1 if blank != 1 else 0, dtype=torch.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _case(name, logits, rows, in_len, blank=0, tgt_len=None, width=None, **meta):
    tl = torch.tensor([len(r) for r in rows] if tgt_len is None else tgt_len, dtype=torch.int64)
    c = dict(name=name, logits=logits, targets=_pad(rows, width, blank), in_len=torch.tensor(in_len, dtype=torch.int64), tgt_len=tl,
             blank=blank, single_path=[], infeasible=[], guarded=[], repeat_at={}, raised_in_len=None, clamped_in_len=None)
    c.update(meta)
    return c


def _waves(name, V, T, seed, blank=0, scale=1.0):
    g = _gen(seed)
    rows = [_labels(g, L, V, blank) for L in WAVE_LENGTHS]
    logits = torch.randn(len(rows), T, V, generator=g) * scale
    return _case(name, logits, rows, [T] * len(rows), blank)


def _straddle(name, off, seed, V=50, T=260):
    """every utterance long enough carries the pair (i, i + 1) equal for i = 31 + off, 63 + off, 95 + off and no other repeat"""
    g = _gen(seed)
    rows, rep = [], {}
    for b, L in enumerate(WAVE_LENGTHS):
        r = _labels(g, L, V, 0, distinct_neighbours=True)
        at = [i + off for i in STRADDLE_AT if i + off + 1 < L]
        for i in at:
            r[i + 1] = r[i]
            if i + 2 < L and int(r[i + 2]) == int(r[i + 1]):          # keep the pair a pair
                r[i + 2] = 1 + (int(r[i + 1]) % (V - 1))
        rows.append(r)
        rep[b] = at
    logits = torch.randn(len(rows), T, V, generator=g)
    return _case(name, logits, rows, [T] * len(rows), 0, repeat_at=rep)


def _single_path(name, short, seed=11, V=50):
    """all labels equal: l _ l _ ... l needs 2L - 1 frames and is the only alignment of that length; one frame fewer has none.
    Utterances 0 and 2 are those (L = 40, 100), 1 and 3 are ordinary neighbours."""
    g = _gen(seed)
    T = 199
    rows = [torch.full((40,), 7, dtype=torch.int64), _labels(g, 70, V, 0), torch.full((100,), 3, dtype=torch.int64), _labels(g, 20, V, 0)]
    logits = torch.randn(4, T, V, generator=g)
    exact = [79, T, 199, 150]
    if not short:
        return _case(name, logits, rows, exact, 0, single_path=[0, 2])
    return _case(name, logits, rows, [78, T, 198, 150], 0, infeasible=[0, 2], raised_in_len=torch.tensor(exact, dtype=torch.int64))


def _empty_and_short(name, seed=12, V=50, T=210):
    g = _gen(seed)
    rows = [_labels(g, 0, V, 0), _labels(g, 100, V, 0, True), _labels(g, 5, V, 0), _labels(g, 0, V, 0), _labels(g, 0, V, 0),
            _labels(g, 1, V, 0), _labels(g, 2, V, 0), _labels(g, 127, V, 0, True)]
    in_len = [T, T, 0, 0, 1, 1, 1, 2 * 127 + 1 - 50]          # 6: two labels in one frame; 7: 127 distinct labels in 205 frames
    logits = torch.randn(len(rows), T, V, generator=g)
    raised = torch.tensor([T, T, 5, 0, 1, 1, 2, in_len[7]], dtype=torch.int64)
    return _case(name, logits, rows, in_len, 0, infeasible=[2, 6], raised_in_len=raised)


def _ragged(name, seed=13, V=50, T=200, B=8):
    g = _gen(seed)
    Ls = [int(x) for x in torch.randint(1, 61, (B,), generator=g)]
    rows = [_labels(g, L, V, 0) for L in Ls]
    in_len = [int(torch.randint(2 * L + 1, T, (1,), generator=g)) for L in Ls]
    in_len[3] = T
    logits = torch.randn(B, T, V, generator=g)
    return _case(name, logits, rows, in_len, 0)


def _in_len_clamp(name, seed=14, V=50, T=150, B=4):
    g = _gen(seed)
    rows = [_labels(g, L, V, 0) for L in (33, 10, 65, 64)]
    logits = torch.randn(B, T, V, generator=g)
    return _case(name, logits, rows, [T + 1, 100, T + 1000, 2 ** 31 - 1], 0,
                 clamped_in_len=torch.tensor([T, 100, T, T], dtype=torch.int64))


def _tgt_len_guard(name, seed=15, V=50, T=140):
    """padded width 40 (Smax = 81): target lengths 41 (one past), 127 (the kernel's own limit, still past this call's), 10 ** 6
    and -1 are outside it; the rows are filled to the full width with valid labels, so a kernel that believed 41 could not
    fault, it would read the neighbour's row"""
    g = _gen(seed)
    W = 40
    rows = [_labels(g, W, V, 0) for _ in range(7)]
    tgt_len = [W, W + 1, 33, 127, 10 ** 6, -1, 40]
    logits = torch.randn(len(rows), T, V, generator=g)
    return _case(name, logits, rows, [T] * len(rows), 0, tgt_len=tgt_len, width=W, guarded=[1, 3, 4, 5],
                 raised_tgt_len=torch.tensor([W, W, 33, W, W, W, 40], dtype=torch.int64))


def _peaked(name, scale, seed):
    g = _gen(seed)
    V, T = 4233, 349
    rows = [_labels(g, L, V, 0) for L in (44, 100, 127, 10)]
    logits = torch.randn(len(rows), T, V, generator=g) * scale
    return _case(name, logits, rows, [T, T, T, 200], 0)


def _aishell(name, seed=20):
    g = _gen(seed)
    B, T, V = 32, 250, 4233
    Ls = [int(x) for x in torch.randint(1, 45, (B,), generator=g)]
    Ls[0], Ls[1] = 44, 1
    rows = [_labels(g, L, V, 0) for L in Ls]
    in_len = [int(torch.randint(max(2 * L + 1, 60), T + 1, (1,), generator=g)) for L in Ls]
    in_len[0] = T
    logits = torch.randn(B, T, V, generator=g)
    return _case(name, logits, rows, in_len, 0)


BUILDERS = {
    'waves_v50': lambda n: _waves(n, 50, 260, 1),
    'waves_v4233': lambda n: _waves(n, 4233, 256, 2),
    'straddle_before': lambda n: _straddle(n, -1, 3),          # pairs on states 61 | 63, 125 | 127, 189 | 191: inside one wave
    'straddle_on': lambda n: _straddle(n, 0, 4),               # 63 | 65, 127 | 129, 191 | 193: across the boundary
    'straddle_after': lambda n: _straddle(n, 1, 5),            # 65 | 67, 129 | 131, 193 | 195
    'single_path': lambda n: _single_path(n, False),
    'one_frame_short': lambda n: _single_path(n, True),
    'empty_and_short': _empty_and_short,
    'ragged_in_len': _ragged,
    'in_len_clamp': _in_len_clamp,
    'tgt_len_guard': _tgt_len_guard,
    'blank_last': lambda n: _waves(n, 50, 260, 6, blank=49),
    'blank_mid': lambda n: _waves(n, 50, 260, 7, blank=25),
    'peaked_x4': lambda n: _peaked(n, 4.0, 8),
    'peaked_x8': lambda n: _peaked(n, 8.0, 9),
    'aishell': _aishell,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: logits f32 [B, T, V], targets int64 [B, W], in_len / tgt_len int64 [B], blank, and what it claims:
    single_path / infeasible / guarded (utterance indices), repeat_at {b: label positions i with labels i, i + 1 equal},
    raised_in_len / raised_tgt_len (the same batch with the infeasible / guarded utterances made feasible), clamped_in_len"""
    return BUILDERS[name](name)


# ------------------------------------------------------------------------------------------ what a case claims
def repeats(case):
    """adjacent equal label pairs inside the first tgt_len_b labels, per utterance (0 for a guarded one)"""
    out = []
    for b in range(case['targets'].shape[0]):
        L = int(case['tgt_len'][b])
        r = case['targets'][b, :L] if 0 <= L <= case['targets'].shape[1] else case['targets'][b, :0]
        out.append(int((r[1:] == r[:-1]).sum()))
    return out


def feasible(case):
    """an alignment exists iff T_b >= L_b + repeats_b (and T_b >= 1 unless there is nothing to align at all: F.ctc_loss gives
    nll 0 for no frames and no labels, which the kernel's zero for 'infeasible' equals); guarded utterances are not feasible"""
    T = case['logits'].shape[1]
    il, tl, guarded = effective_lengths(case['targets'], case['in_len'], case['tgt_len'], T)
    rep = repeats(case)
    return [bool(not guarded[b] and int(il[b]) >= 1 and int(il[b]) >= int(tl[b]) + rep[b]) for b in range(len(rep))]


def single_path_closed_form(case, b):
    """float64 (nll_b, slab_b) of an utterance whose labels are all equal with T_b = 2 L_b - 1: the alignment l _ l _ ... l,
    nll = - sum_t lp[t, path_t], gradient coef_b * (softmax - onehot(path_t)) on its frames and zero after them"""
    lp = F.log_softmax(case['logits'][b].double(), -1)
    T, V = lp.shape
    Tb, L = int(case['in_len'][b]), int(case['tgt_len'][b])
    assert Tb == 2 * L - 1
    path = torch.full((Tb,), case['blank'], dtype=torch.int64)
    path[0::2] = case['targets'][b, 0]
    nll = -lp[torch.arange(Tb), path].sum()
    g = torch.zeros(T, V, dtype=torch.float64)
    g[:Tb] = lp[:Tb].exp()
    g[torch.arange(Tb), path] -= 1.0
    return nll, g * coef(case['tgt_len'], case['targets'], case['logits'].shape[0])[b]


# ------------------------------------------------------------------------------------------ cached per case (both test files)
@functools.lru_cache(maxsize=None)
def reference_of(name):
    c = build(name)
    return reference(c['logits'], c['targets'], c['in_len'], c['tgt_len'], c['blank'])


@functools.lru_cache(maxsize=None)
def floor_of(name):
    c = build(name)
    return floor(c['logits'], c['targets'], c['in_len'], c['tgt_len'], c['blank'], ref=reference_of(name))


@functools.lru_cache(maxsize=None)
def tiny_of(name):
    c = build(name)
    return tiny(c['logits'], c['in_len'])
