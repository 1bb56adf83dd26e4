"""The case lists of tests/test_nbest_consensus.py (CPU, the restatement alone) and tests/test_gpu_nbest_consensus.py (the kernels against
it): not a test.  Everything here is a pure function of its arguments."""
import math

import numpy as np

INF = float('inf')
GRID = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256)      # lengths around the 64-column chunk of a wave, its multiples, the limit
MAX_LEN = 256                                              # ops.NBEST_MAX_LEN, asserted by the tests
ALPHABET = 4                                               # few symbols: the three predecessors tie often, where a wrong preference shows


def align_grid(seed=4):
    """all 121 (reference, hypothesis) length pairs of GRID as one B = 121, N = 1 batch: (ref, ref_len, hyp, hyp_len)"""
    rng = np.random.default_rng(seed)
    n = len(GRID)
    rl, hl = np.repeat(GRID, n), np.tile(GRID, n)
    r = rng.integers(0, ALPHABET, size=(n * n, MAX_LEN))
    h = rng.integers(0, ALPHABET, size=(n * n, 1, MAX_LEN))
    return r, rl, h, hl.reshape(n * n, 1)


# hand-made n-bests: tokens (ragged lists), scores, scale, and what the definition gives, worked out by hand
HAND = [
    dict(name='identical', tokens=[[1, 2, 3]] * 3, scores=[0.0, -1.0, -2.0], scale=1.0,
         post=None, risk=[0.0, 0.0, 0.0], best=0, conf=[[1.0, 1.0, 1.0]] * 3),
    dict(name='one_substitution', tokens=[[1, 2, 3], [1, 4, 3]], scores=[math.log(3.0), 0.0], scale=1.0,
         post=[0.75, 0.25], risk=[0.25, 0.75], best=0, conf=[[1.0, 0.75, 1.0], [1.0, 0.25, 1.0]]),
    dict(name='one_substitution_scaled', tokens=[[1, 2, 3], [1, 4, 3]], scores=[0.0, 2 * math.log(3.0)], scale=0.5,
         post=[0.25, 0.75], risk=[0.75, 0.25], best=1, conf=[[1.0, 0.25, 1.0], [1.0, 0.75, 1.0]]),
    # [1, 2] against the empty reference: two insertions; the empty one against [1, 2]: two deletions, no token.  Equal risks, equal
    # scores: the lower index
    dict(name='empty_hypothesis', tokens=[[1, 2], []], scores=[0.0, 0.0], scale=1.0,
         post=[0.5, 0.5], risk=[1.0, 1.0], best=0, conf=[[0.5, 0.5], [0.0, 0.0]]),
    dict(name='one_live_slot', tokens=[[7, 7], [1, 2], [3]], scores=[-INF, 0.3, -INF], scale=1.0,
         post=[0.0, 1.0, 0.0], risk=[INF, 0.0, INF], best=1, conf=[[0.0, 0.0], [1.0, 1.0], [0.0, 0.0]]),
    dict(name='no_live_slot', tokens=[[1, 2], [1, 3]], scores=[-INF, float('nan')], scale=1.0,
         post=[0.0, 0.0], risk=[INF, INF], best=-1, conf=[[0.0, 0.0], [0.0, 0.0]]),
    # the dead slot in the middle adds nothing; 0 and 2 tie on risk and score: the lower index
    dict(name='minus_inf_in_the_middle', tokens=[[1, 2, 3], [9, 9, 9], [1, 2, 4]], scores=[0.0, -INF, 0.0], scale=1.0,
         post=[0.5, 0.0, 0.5], risk=[0.5, INF, 0.5], best=0, conf=[[1.0, 1.0, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, 0.5]]),
    # 0 and 1 are the same string, so their risks are equal and the lowest; 1 scores higher: the tie goes to it
    dict(name='tie_to_the_higher_score', tokens=[[1, 2], [1, 2], [5, 6, 7]], scores=[0.0, 1.0, 0.5], scale=1.0,
         post=None, risk=None, best=1, conf=None),
]


def hand_arrays(case):
    """(tokens int64 [1, N, L], lengths int32 [1, N], scores f32 [1, N]) of a HAND case, padded with -1"""
    toks = case['tokens']
    L = max(max(len(t) for t in toks), 1)
    tokens = np.full((1, len(toks), L), -1, np.int64)
    for n, t in enumerate(toks):
        tokens[0, n, :len(t)] = t
    return tokens, np.array([[len(t) for t in toks]], np.int32), np.array([case['scores']], np.float32)


# (name, B, N, the lengths a slot draws from, scale, seed): N in {1, 2, 3, 10, 32}, B in {1, 5}, the grid and the limit; the wide
# n-bests keep to the shorter lengths so that the float64 restatement of each case stays a matter of seconds
CONSENSUS = [
    ('n1', 5, 1, (0, 1, 65, 129, 256), 1.0, 1),
    ('n2_limit', 1, 2, (255, 256), 1.0, 23),
    ('n2_grid', 5, 2, GRID, 0.5, 3),
    ('n3_long', 5, 3, (127, 128, 129, 255, 256), 1.0, 4),
    ('n10', 1, 10, (2, 63, 64, 65, 127, 128, 129), 2.0, 5),
    ('n32', 5, 32, (0, 1, 2, 63, 64, 65), 1.0, 6),
    ('n32_b1', 1, 32, (1, 2, 63, 64, 65, 127, 128), 0.3, 7),
]


def consensus_inputs(B, N, lens, seed, dead=True):
    """A random n-best per utterance: every hypothesis is one base string with about 15 % of its tokens substituted, a few dropped and
    a few inserted, cut or filled to a length drawn from `lens`; normal scores.  With `dead`, about one slot in six is dead, by a -inf
    score, a nan score, or a length outside the width.  -> (tokens int64 [B, N, L], lengths int32 [B, N], scores f32 [B, N]); the
    padding holds -1."""
    rng = np.random.default_rng(seed)
    L = max(max(lens), 1)
    tokens = np.full((B, N, L), -1, np.int64)
    lengths = np.zeros((B, N), np.int32)
    scores = (rng.standard_normal((B, N)) * 2.0).astype(np.float32)
    for b in range(B):
        base = rng.integers(0, ALPHABET, size=L)
        for n in range(N):
            h = base.copy()
            sub = rng.random(L) < 0.15
            h[sub] = rng.integers(0, ALPHABET, size=int(sub.sum()))
            h = h[rng.random(L) >= 0.05]
            for _ in range(int(rng.integers(0, 4))):
                h = np.insert(h, int(rng.integers(0, len(h) + 1)), int(rng.integers(0, ALPHABET)))
            H = int(rng.choice(lens))
            h = np.concatenate([h, rng.integers(0, ALPHABET, size=L)])[:H]
            tokens[b, n, :H] = h
            lengths[b, n] = H
            if dead and N > 1 and rng.random() < 1 / 6:
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    scores[b, n] = -INF
                elif kind == 1:
                    scores[b, n] = np.nan
                else:
                    lengths[b, n] = (-1, L + 1)[int(rng.integers(0, 2))]
    return tokens, lengths, scores


def clear_of_near_ties(risk, scores, live):
    """the condition the comparison of `best` rests on: in the restatement the two lowest risks of every utterance differ by more than
    1e-3, or are exactly equal (then the tie rules decide: scores or indices, which always differ)"""
    for b in range(risk.shape[0]):
        r = sorted(float(risk[b, n]) for n in range(risk.shape[1]) if live[b, n])
        if len(r) >= 2 and r[0] != r[1] and r[1] - r[0] <= 1e-3:
            return False
    return True


# calibration by hand: four tokens, confidences 0.9, 0.8, 0.3, 0.6, outcomes 1, 1, 0, 0
CALIBRATION = dict(conf=[0.9, 0.8, 0.3, 0.6], correct=[1, 1, 0, 0])
_hp = -(2 * math.log(0.5) + 2 * math.log(0.5))
_hc = -(math.log(0.9) + math.log(0.8) + math.log(0.7) + math.log(0.4))
CALIBRATION['nce'] = (_hp - _hc) / _hp
# bins [0.3, 0.4): one token, outcome 0, gap 0.3; [0.6, 0.7): one, outcome 0, gap 0.6; [0.8, 0.9): one, outcome 1, gap 0.2; [0.9, 1]:
# one, outcome 1, gap 0.1; each weighs 1 / 4
CALIBRATION['ece'] = (0.3 + 0.6 + 0.2 + 0.1) / 4
