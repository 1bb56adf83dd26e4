"""Dict-based float64 restatement of the backoff rule of include/otrans_hip.h (the n-gram LM of otr_ngram_lookup and
otr_ctc_beam_search_lm), and the helper that writes the ARPA files the n-gram tests load.

RefLM holds {n-gram tuple: (log-prob, backoff)} with the very f32-rounded natural-log values the loader stores, so the device and
this file differ in summation only (f32 there, float64 here)."""
import math

import numpy as np

LN10 = math.log(10.0)


def f32(log10_value):
    """what NGramLM.from_arpa stores for a log10 field: the float64 product with ln 10, rounded to f32 once"""
    return float(np.float32(float(log10_value) * LN10))


class RefLM:
    def __init__(self, grams, order, V, oov_score=-1000.0):
        self.grams, self.order, self.V, self.oov_score = grams, order, V, oov_score

    def context(self, prefix):
        """<s> followed by the prefix, cut to its last order-1 ids"""
        full = (self.V,) + tuple(prefix)
        return full[len(full) - min(len(full), self.order - 1):] if self.order > 1 else ()

    def cond(self, ctx, c):
        """ln P(c | ctx): ctx a tuple of at most order-1 ids"""
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        if (c,) not in self.grams or any((w,) not in self.grams for w in ctx):
            return self.oov_score
        acc = 0.0
        for k in range(len(ctx), -1, -1):
            h = ctx[len(ctx) - k:]
            e = self.grams.get(h + (c,))
            if e is not None:
                return acc + e[0]
            if k and h in self.grams:
                acc += self.grams[h][1]
        raise AssertionError('unreachable: the unigram is stored')

    def score(self, string):
        """ln P_LM(string) = sum over its tokens of ln P(token | context of what precedes it)"""
        return sum(self.cond(self.context(string[:j]), string[j]) for j in range(len(string)))


def make_lm(seed, V, order, per_order, absent=(), eos_unit=1, unk_unit=None):
    """A random backoff LM over units [0, V): returns (ARPA text, {n-gram: (lp, bo)} as the loader stores them, idx2unit).
    The n-gram set is closed under prefix and suffix; the file has <s>, </s> (= eos_unit), <unk> (= unk_unit, or dropped), one
    unigram whose word has no unit (dropped), entries with and without a backoff field; unit 0 (blank) and `absent` are left out.
    per_order: how many 2-grams, 3-grams, ... to draw (fewer if the closure cannot supply them)."""
    rng = np.random.default_rng(seed)
    idx2unit = {i: 'u%d' % i for i in range(V)}

    def word(i):
        return '<s>' if i == V else '</s>' if i == eos_unit else '<unk>' if i == unk_unit else idx2unit[i]
    units = [i for i in range(1, V) if i not in absent]
    sets = [[(i,) for i in units] + [(V,)]]
    for m in range(2, order + 1):
        prev = sets[-1]
        by_prefix = {}
        for h in prev:
            if h[-1] != V:
                by_prefix.setdefault(h[:-1], []).append(h)
        new = set()
        want = per_order[m - 2]
        for _ in range(8):                             # a few passes: one random extension of every (m-1)-gram per pass
            for gi in rng.permutation(len(prev)):
                hs = by_prefix.get(prev[gi][1:])
                if hs and len(new) < want:
                    new.add(prev[gi] + (hs[rng.integers(len(hs))][-1],))
        sets.append(sorted(new))
    grams, lines = {}, ['\\data\\'] + ['ngram %d=%d' % (m + 1, len(s) + (2 if m == 0 and unk_unit is None else 1 if m == 0 else 0))
                                        for m, s in enumerate(sets)]
    for m, s in enumerate(sets, 1):
        lines += ['', '\\%d-grams:' % m]
        if m == 1:
            lines.append('-1.5\tnot_a_unit\t-0.25')
            if unk_unit is None:
                lines.append('-2.5\t<unk>\t-0.125')
        for g in s:
            lp = -99.0 if g == (V,) else -round(float(rng.uniform(0.1, 3.0)), 4)
            bo = None if m == order or (g != (V,) and rng.random() < 0.3) else -round(float(rng.uniform(0.0, 1.0)), 4)
            grams[g] = (f32(lp), f32(bo) if bo is not None else 0.0)
            lines.append('%s\t%s' % (repr(lp), ' '.join(word(i) for i in g)) + ('' if bo is None else '\t%s' % repr(bo)))
    lines += ['', '\\end\\', '']
    return '\n'.join(lines), grams, idx2unit
