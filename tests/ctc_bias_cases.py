"""The inputs of the device comparisons of the phrase-biased CTC prefix beam search (tests/test_gpu_ctc_bias.py), shared with the CPU
test (tests/test_ctc_bias.py) that asserts, on the restatement alone, what the GPU tests rely on: each case leaves at least
`min_clear` utterances clear of a W/W+1 near-tie, the planted case walks a chain of depth 16, fails over from one phrase to another,
refunds an open match at the end of an utterance and reorders a beam by it, and the golden case holds a hypothesis that only the
biased search keeps.  Everything is computed once per process."""
import functools

import numpy as np

from tests import ctc_prefix_bias_ref as bref
from tests import ctc_prefix_ref as plain_ref
from tests import ngram_cases
from tests.bias_ref import RefBias
from tests.ngram_cases import ALPHA, BETA, GOLDEN_KS, GOLDEN_LENGTHS, GOLDEN_WS, clear_count, golden_log_probs   # noqa: F401

GAP = 1e-4                                   # the project's value (ngram_cases.GAP)
EOS, BLANK = 1, 0
WEIGHTS = (0.5, 1.0, 1.5, 2.0, 3.0)          # dyadic: every sum of addends is exact in f32
GOLDEN_SEED, PLANTED_SEED = 2, 0
GOLDEN_V = 100
P_B, P_T, P_V, P_W, P_K = 5, 64, 4233, 10, 40
MODEL_LENGTHS = [12, 20, 35, 11]             # the frames the C1 model's frontend leaves of c1_decode.npz's four utterances
LENGTH_SETS = tuple(GOLDEN_LENGTHS) + (MODEL_LENGTHS,)
# the "brought back" hypothesis: (index into LENGTH_SETS, utterance, W, K); tests/test_ctc_bias.py asserts that the biased W-best
# of that utterance holds a hypothesis the unbiased W-best does not, and names the phrase that pays for it
BROUGHT_BACK = (2, 0, 5, 40)
BROUGHT_BACK_HYP = (37, 79, 64, 56, 56, 1)


def pair(phrases, weights, V):
    """(PhraseBias, RefBias) over the same phrases"""
    from opentransformer_amd.bias import PhraseBias
    return PhraseBias(phrases, V, weights=weights, eos_unit=EOS), RefBias(phrases, weights, V, EOS)


# ------------------------------------------------------------------ the golden case: tests/golden/c1_decode.npz, V = 100
@functools.lru_cache(maxsize=None)
def golden_phrases():
    """about 60 phrases: 2-6-unit substrings of ranks 2-5 of the plain W = 5 search (none holding unit 0 or 1), 40 random phrases of
    1-16 ids in [2, 100), one phrase that is a prefix of another and one that shares a two-unit prefix with another"""
    rng = np.random.default_rng(GOLDEN_SEED)
    lp = golden_log_probs()
    phrases = []
    for b in range(lp.shape[0]):
        hyps = plain_ref.decode_one(lp[b].astype(np.float64), GOLDEN_LENGTHS[0][b], 5, 40)
        for s, _ in hyps[1:5]:
            for _ in range(8):                                   # a few tries per hypothesis
                n = int(rng.integers(2, 7))
                if len(s) < n:
                    continue
                o = int(rng.integers(0, len(s) - n + 1))
                sub = tuple(s[o:o + n])
                if 0 in sub or 1 in sub or sub in phrases:
                    continue
                phrases.append(sub)
                break
    for _ in range(40):
        phrases.append(tuple(int(v) for v in rng.integers(2, GOLDEN_V, size=int(rng.integers(1, 17)))))
    longest = max(phrases[:16], key=len)
    phrases.append(longest[:-1] if len(longest) > 2 else longest + (int(rng.integers(2, GOLDEN_V)),))      # a prefix of / an extension of it
    phrases.append(longest[:2] + (int(rng.integers(2, GOLDEN_V)),))                                        # shares its first two units
    phrases = list(dict.fromkeys(phrases))
    weights = [float(WEIGHTS[int(rng.integers(len(WEIGHTS)))]) for _ in phrases]
    return tuple(phrases), tuple(weights)


@functools.lru_cache(maxsize=None)
def golden_bias():
    phrases, weights = golden_phrases()
    return pair(list(phrases), list(weights), GOLDEN_V)


@functools.lru_cache(maxsize=None)
def golden_reference(W, K, with_ngram, which):
    """(tokens, out_len, scores, lm_scores, bias_scores, gaps, refunds) of the restatement on the golden log-probs with
    LENGTH_SETS[which]; with_ngram: ngram_cases.golden_lm(3) at ALPHA / BETA"""
    gaps, refunds = [], []
    lm = ngram_cases.golden_lm(3)[1] if with_ngram else None
    out = bref.decode(golden_log_probs(), LENGTH_SETS[which], W, K, golden_bias()[1], lm, ALPHA if with_ngram else 0.0,
                      BETA if with_ngram else 0.0, min_gap=gaps, refunds=refunds)
    return out + (gaps, refunds)


@functools.lru_cache(maxsize=None)
def golden_plain(W, K, which):
    """the unbiased search of the same inputs (tests/ctc_prefix_ref)"""
    return plain_ref.decode(golden_log_probs(), LENGTH_SETS[which], W, K)


# ------------------------------------------------------------------ the planted case: V = 4233, chains, fail-over, refunds
@functools.lru_cache(maxsize=None)
def planted():
    """dict(lp f32 [5, 64, 4233], lengths, phrases, weights, spelled: the unit strings the frames spell, named: the phrases with a
    role).  Frames: log_softmax of N(0, 1) noise plus 9.0 on the planted label and 6.5 on one random rival; a planted unit holds two
    frames and a blank frame follows it."""
    import torch
    rng = np.random.default_rng(PLANTED_SEED)
    ids = [int(v) for v in rng.permutation(np.arange(2, P_V))[:64]]           # distinct ids for the named phrases and the foreign units
    assert max(ids) > 4096 and sum(v > 255 for v in ids) > 32
    P16 = tuple(ids[:16])
    a1, a2, a3, a4, x = ids[16:21]
    A, A2, A3 = (a1, a2, a3, a4), (a2, a3, x), (a1, a2)
    D = tuple(ids[21:25])
    z, q = ids[25:27]
    Z = (z, z, q)
    f = ids[27:40]                                                            # foreign units: in no phrase
    named = dict(P16=P16, A=A, A2=A2, A3=A3, D=D, Z=Z)
    phrases = list(named.values())
    taken = set(ids)
    while len(phrases) < 60:                                                  # random phrases of 1-8 ids that avoid the ids above
        p = tuple(int(v) for v in rng.integers(2, P_V, size=int(rng.integers(1, 9))))
        if not taken & set(p):
            phrases.append(p)
    weights = [float(WEIGHTS[int(rng.integers(len(WEIGHTS)))]) for _ in phrases]
    spelled = [P16,                                                           # P16 completed
               (f[0],) + P16[:15] + (f[1],),                                  # 15 of its 16 ids between foreign units: all refunded
               (a1, a2, a3, x, f[2], f[3]),                                   # the match fails over from A to (a2, a3, x)
               (f[4], f[5]) + D[:3],                                          # ends inside D: the refund after the last frame
               (z, z) + A + (f[6],)]                                          # a doubled unit in front of A: the 1b merge with an addend
    lengths = [P_T, P_T, P_T, 15, P_T]
    x_ = rng.normal(size=(P_B, P_T, P_V)).astype(np.float32)
    for b, s in enumerate(spelled):
        label = []
        for u in s:
            label += [u, u, BLANK]
        label += [BLANK] * (P_T - len(label))
        for t in range(P_T):
            x_[b, t, label[t]] += 9.0
            x_[b, t, int(rng.integers(0, P_V))] += 6.5
    lp = torch.log_softmax(torch.from_numpy(x_), -1).numpy()
    return dict(lp=lp, lengths=lengths, phrases=phrases, weights=weights, spelled=spelled, named=named)


@functools.lru_cache(maxsize=None)
def planted_bias():
    p = planted()
    return pair(p['phrases'], p['weights'], P_V)


@functools.lru_cache(maxsize=None)
def planted_reference():
    """as golden_reference, without an n-gram"""
    p = planted()
    gaps, refunds = [], []
    out = bref.decode(p['lp'], p['lengths'], P_W, P_K, planted_bias()[1], min_gap=gaps, refunds=refunds)
    return out + (gaps, refunds)
