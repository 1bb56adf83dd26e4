"""tests/ctc_prefix_ref.py's prefix beam search with the n-gram LM addend of include/otrans_hip.h (otr_ctc_beam_search_lm), float64:
every contribution to pnb'(s+c) gains a(s+c) = alpha * ln P_LM(c | context(s)) + beta, whether it creates s+c or merges into an s+c
already in the beam; blank and repeat stays gain nothing.  Each string also carries the sum of its addends (lm_scores)."""
import math

import numpy as np

from tests.ctc_prefix_ref import NEG_INF, lae, topk


def decode_one(lp, length, W, K, lm, alpha, beta, blank=0, gaps=None):
    """lp [T, V], lm a tests.ngram_ref.RefLM -> list of (tokens tuple, score, lm score) in beam order; `gaps` as in ctc_prefix_ref"""
    addend = {}

    def a(s, c):
        key = (lm.context(s), c)
        v = addend.get(key)
        if v is None:
            v = addend[key] = alpha * lm.cond(key[0], c) + beta
        return v
    beam = [((), 0.0, NEG_INF)]
    lms = {(): 0.0}
    for t in range(length):
        cands = topk(lp[t], K)
        new = {}

        def entry(s, key):
            e = new.get(s)
            if e is None:
                e = new[s] = [NEG_INF, NEG_INF, key]
            return e
        in_beam = {s: i for i, (s, _, _) in enumerate(beam)}
        for i, (s, pb, pnb) in enumerate(beam):
            entry(s, (i, -1))
        for i, (s, pb, pnb) in enumerate(beam):
            last = s[-1] if s else None
            for p, c in cands:
                if c == blank:
                    e = new[s]
                    e[0] = lae(e[0], lae(pb, pnb) + p)
                    continue
                if c == last:
                    e = new[s]
                    e[1] = lae(e[1], pnb + p)
                    base = pb
                else:
                    base = lae(pb, pnb)
                s2 = s + (c,)
                add = a(s, c)
                if s2 not in lms:
                    lms[s2] = lms[s] + add
                e = entry(s2, (in_beam[s2], -1) if s2 in in_beam else (i, c))
                e[1] = lae(e[1], base + p + add)
        scored = [(lae(pb, pnb), key, s, pb, pnb) for s, (pb, pnb, key) in new.items()]
        scored = [x for x in scored if x[0] > NEG_INF]
        scored.sort(key=lambda x: (-x[0], x[1]))
        if gaps is not None:
            gaps.append(scored[W - 1][0] - scored[W][0] if len(scored) > W else math.inf)
        beam = [(s, pb, pnb) for _, _, s, pb, pnb in scored[:W]]
        lms = {s: lms[s] for s, _, _ in beam}
        if not beam:
            break
    return [(s, lae(pb, pnb), lms[s]) for s, pb, pnb in beam]


def decode(log_probs, lengths, W, K, lm, alpha, beta, blank=0, min_gap=None):
    """log_probs [B, T, V] -> tokens int64 [B, W, T] (-1 padded), out_len int32 [B, W], scores [B, W], lm_scores [B, W] (float64),
    laid out as the kernel's outputs; `min_gap` receives each utterance's smallest W/W+1 boundary gap"""
    log_probs = np.asarray(log_probs, dtype=np.float64)
    B, T, V = log_probs.shape
    K = min(K, V)
    tokens = -np.ones((B, W, T), np.int64)
    out_len = np.zeros((B, W), np.int32)
    scores = np.full((B, W), NEG_INF)
    lm_scores = np.zeros((B, W))
    for b in range(B):
        g = []
        hyps = decode_one(log_probs[b], min(max(int(lengths[b]), 0), T), W, K, lm, alpha, beta, blank, g)
        if min_gap is not None:
            min_gap.append(min(g, default=math.inf))
        for r, (s, sc, ls) in enumerate(hyps):
            tokens[b, r, :len(s)] = s
            out_len[b, r] = len(s)
            scores[b, r] = sc
            lm_scores[b, r] = ls
    return tokens, out_len, scores, lm_scores
