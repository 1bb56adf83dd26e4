"""The n-gram estimator of NGramLM.train (include/otrans_hip.h, the estimation section) restated with Python dicts: interpolated
modified Kneser-Ney with KenLM's <s> rule.  Independent of the package: it shares no code with opentransformer_amd/ngram.py or the
kernels of csrc/ngramtrain.hip, only the written rule.  Grams are tuples of ids, oldest first; V is <s>, eos is </s>."""
import math
from collections import defaultdict

import numpy as np

FALLBACK = (0.5, 1.0, 1.5)


def raw_counts(sents, order, V, eos=1):
    """{gram: count} of every m-gram, m = 1 .. order, that ends at a position of <s> w_1 .. w_n </s>"""
    c = defaultdict(int)
    for s in sents:
        x = [V] + [int(w) for w in s] + [eos]
        for i in range(len(x)):
            for m in range(1, min(order, i + 1) + 1):
                c[tuple(x[i - m + 1:i + 1])] += 1
    return dict(c)


def estimate(sents, order, V, eos=1, units=None, discounts=None):
    """-> dict(counts, logp {gram: f32}, backoff {gram: f32}, discounts [order][3], fallback_orders [m, ...], prob {gram: float})"""
    U = sorted(range(1, V)) if units is None else sorted(int(u) for u in units)
    c = raw_counts(sents, order, V, eos)
    left = defaultdict(set)                                  # gram -> the ids that precede it somewhere
    for g in c:
        if len(g) > 1:
            left[g[1:]].add(g[0])
    a = {}
    for g, n in c.items():
        if g == (V,):
            continue
        a[g] = n if len(g) == order or g[0] == V else len(left[g])
    ctx = defaultdict(lambda: [0, 0, 0, 0])                  # sum, n1, n2, n3p
    nn = [[0] * 5 for _ in range(order + 1)]
    for g, n in a.items():
        st = ctx[g[:-1]]
        st[0] += n
        st[min(n, 3)] += 1
        if n <= 4:
            nn[len(g)][n] += 1
    fallback, D = [], []
    for m in range(1, order + 1):
        n1, n2, n3, n4 = nn[m][1:5]
        d = None
        if min(n1, n2, n3, n4) > 0:
            Y = n1 / (n1 + 2.0 * n2)
            d = (1 - 2 * Y * n2 / n1, 2 - 3 * Y * n3 / n2, 3 - 4 * Y * n4 / n3)
            if not all(0.0 <= d[k] <= k + 1 for k in range(3)):
                d = None
        if d is None:
            fallback.append(m)
            d = FALLBACK
        D.append(tuple(d))
    if discounts is not None:
        D, fallback = [tuple(float(v) for v in row) for row in discounts], []

    def gamma(h, m):                                         # the interpolation weight of context h for grams of order m
        s, n1, n2, n3p = ctx[h]
        return (D[m - 1][0] * n1 + D[m - 1][1] * n2 + D[m - 1][2] * n3p) / s

    prob = {}
    for m in range(1, order + 1):
        for g, n in a.items():
            if len(g) != m:
                continue
            lower = 1.0 / len(U) if m == 1 else prob[g[1:]]
            prob[g] = (n - D[m - 1][min(n, 3) - 1]) / ctx[g[:-1]][0] + gamma(g[:-1], m) * lower
    for u in U:
        if (u,) not in prob:
            prob[(u,)] = gamma((), 1) / len(U)
    logp = {g: np.float32(math.log(p)) for g, p in prob.items()}
    logp[(V,)] = np.float32(-99.0 * math.log(10.0))
    backoff = {}
    for g in logp:
        has = len(g) < order and g in ctx and ctx[g][0] > 0
        backoff[g] = np.float32(math.log(gamma(g, len(g) + 1))) if has else np.float32(0.0)
    return dict(counts=c, logp=logp, backoff=backoff, discounts=D, fallback_orders=fallback, prob=prob, contexts=dict(ctx))


def cond_logp(est, order, ctx, w):
    """ln P(w | ctx) by the backoff rule of include/otrans_hip.h on the restatement's f32 values, summed in f32 longest first"""
    ctx = tuple(ctx)[-(order - 1):] if order > 1 else ()
    acc = np.float32(0.0)
    for k in range(len(ctx), -1, -1):
        g = ctx[len(ctx) - k:] + (w,)
        if g in est['logp']:
            return np.float32(acc + est['logp'][g])
        h = ctx[len(ctx) - k:]
        if k and h in est['backoff']:
            acc = np.float32(acc + est['backoff'][h])
    raise KeyError(w)


def sentence_logp(est, order, V, sent, eos=1):
    """sum of ln P over w_1 .. w_n </s>, each given <s> and what precedes it, in float64 of the f32 terms"""
    hist, tot = [V], 0.0
    for w in list(sent) + [eos]:
        tot += float(cond_logp(est, order, hist, int(w)))
        hist.append(int(w))
    return tot


def arrays(est, order):
    """(ids [n, order] left aligned, lens, logp, backoff) sorted by (order, gram): what the NGramLM constructor takes"""
    grams = sorted(est['logp'], key=lambda g: (len(g), g))
    ids = np.zeros((len(grams), order), np.int64)
    for r, g in enumerate(grams):
        ids[r, :len(g)] = g
    return (ids, np.array([len(g) for g in grams], np.int64), np.array([est['logp'][g] for g in grams], np.float32),
            np.array([est['backoff'][g] for g in grams], np.float32))


def random_corpus(seed, n, V, max_len, eos=1, zipf=None):
    """n sentences of lengths 0 .. max_len over the ids of [1, V) without eos"""
    rng = np.random.default_rng(seed)
    ids = np.array([u for u in range(1, V) if u != eos])
    out = []
    for _ in range(n):
        k = int(rng.integers(0, max_len + 1))
        if zipf:
            r = np.minimum(rng.zipf(zipf, size=k), len(ids)) - 1
        else:
            r = rng.integers(0, len(ids), size=k)
        out.append([int(v) for v in ids[r]])
    return out
