"""numpy float64 restatement of the feature-preparation chain as include/otrans_hip.h states it (otr_feature_prepare,
otr_cmvn_accumulate): not a test.  The chain is the reference's (otrans/data/audio.py:125-136): normalisation -> gaussian noise ->
SpecAugment per utterance, then zero padding to [B, Tmax, F]."""
import numpy as np

EPS32 = 2.0 ** -23


def utterance_stats(x):
    """(mean, unbiased std) over ALL values of x [T, F], in float64 (torch.std_mean(feature) of audio.py:22-24)"""
    x = np.asarray(x, np.float64)
    return float(x.mean()), float(x.std(ddof=1)) if x.size > 1 else float('nan')


def chain(x, norm=None, gmean=None, gstd=None, noise=None, rects=None):
    """one utterance [T, F] -> float64 [T, F]: norm None | 'utterance' | 'global', + noise [F] on every frame, rectangles
    (t0, t1, f0, f1) half-open zeroed last"""
    y = np.asarray(x, np.float64).copy()
    if norm == 'utterance':
        mean, std = utterance_stats(x)
        y = (y - mean) / std
    elif norm == 'global':
        y = (y - np.asarray(gmean, np.float64)) / np.asarray(gstd, np.float64)
    else:
        assert norm is None
    if noise is not None:
        y = y + np.asarray(noise, np.float64)[None, :]
    T, F = y.shape
    for t0, t1, f0, f1 in (rects if rects is not None else ()):
        y[max(t0, 0):max(t1, 0), max(f0, 0):max(f1, 0)] = 0.0
    return y


def prepare(utts, Tmax, norm=None, gmean=None, gstd=None, noise=None, ranges=None):
    """utts: list of [T_b, F] float32 arrays (T_b may be 0 or exceed Tmax: clamped).  Returns dict(dst f64 [B, Tmax, F], mask bool
    [B, Tmax], stats f64 [B, 2], bound f64 [B, Tmax, F]): `bound` is the tolerance of a float32 implementation,
    2 * 2^-23 * (|y| + |mean| / std + 1) for 'utterance' and 2 * 2^-23 * (|y| + 1) otherwise -- half an ulp each for the mean, the
    std, the subtraction and the division is under 2^-23 * (1.5 |y| + 0.5 |mean| / std); twice that leaves room for the order of
    float32 operations and no more.  Where dst is exactly zero by construction (padding, rectangles) the bound is 0."""
    B, F = len(utts), utts[0].shape[1]
    dst = np.zeros((B, Tmax, F))
    bound = np.zeros((B, Tmax, F))
    mask = np.zeros((B, Tmax), bool)
    stats = np.full((B, 2), np.nan)
    for b, x in enumerate(utts):
        n = min(x.shape[0], Tmax)
        if n == 0:
            continue
        x = x[:n]
        rects = None if ranges is None else [tuple(int(v) for v in r) for r in ranges[b]]
        y = chain(x, norm, gmean, gstd, None if noise is None else noise[b], rects)
        extra = 0.0
        if norm == 'utterance':
            stats[b] = utterance_stats(x)
            extra = abs(stats[b, 0]) / stats[b, 1]
        dst[b, :n] = y
        mask[b, :n] = True
        bd = 2 * EPS32 * (np.abs(y) + extra + 1.0)
        zero = np.zeros((n, F), bool)
        for t0, t1, f0, f1 in (rects or ()):
            zero[max(t0, 0):max(t1, 0), max(f0, 0):max(f1, 0)] = True
        bd[zero] = 0.0
        bound[b, :n] = bd
    return dict(dst=dst, mask=mask, stats=stats, bound=bound)


def zero_cells(lengths, Tmax, F, ranges=None):
    """bool [B, Tmax, F]: the cells that must be bit-exact 0.0 (padding and rectangles)"""
    B = len(lengths)
    z = np.zeros((B, Tmax, F), bool)
    for b, n in enumerate(lengths):
        n = min(max(int(n), 0), Tmax)
        z[b, n:] = True
        for t0, t1, f0, f1 in (ranges[b] if ranges is not None else ()):
            z[b, max(t0, 0):min(max(t1, 0), n), max(f0, 0):max(f1, 0)] = True
    return z


def cmvn_sums(utts):
    """float64 [2F + 1]: per-dimension sums, sums of squares, frame count over all frames of utts"""
    F = utts[0].shape[1]
    acc = np.zeros(2 * F + 1)
    for x in utts:
        x = np.asarray(x, np.float64)
        acc[:F] += x.sum(0)
        acc[F:2 * F] += (x * x).sum(0)
        acc[2 * F] += x.shape[0]
    return acc


def cmvn_result(acc):
    """(mean, population std) from the sums: sqrt(max(E[x^2] - mean^2, 0)), Kaldi's convention"""
    F = (len(acc) - 1) // 2
    n = acc[2 * F]
    mean = acc[:F] / n
    return mean, np.sqrt(np.maximum(acc[F:2 * F] / n - mean * mean, 0.0))
