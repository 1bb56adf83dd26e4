"""tests/ctc_prefix_lm_ref.py's prefix beam search with the phrase-biasing addend of include/otrans_hip.h (otr_ctc_beam_search_bias)
beside the optional n-gram addend, float64 for the search, tests/bias_ref.RefBias's f32 for the phrase addends: every contribution
to pnb'(s+c) gains  alpha * ln P_LM(c | context(s)) + beta  (where an LM is given)  +  psi_minus(state(s c)) - psi(state(s)),
whether it creates s+c or merges into an s+c already in the beam; blank and repeat stays gain nothing.  After the last frame every
hypothesis h loses psi(state(h)) -- the refund of a match left open -- and the beam is sorted again, stably.  Each string carries
the sums of its two kinds of addends.  Does not import opentransformer_amd.bias."""
import math

import numpy as np

from tests.ctc_prefix_ref import NEG_INF, lae, topk

F32 = np.float32


def phrase_addend(rb, s, c, memo):
    """rb.addend(s, c) as a float.  A unit that is in no phrase leads to the root, so its addend is 0 - psi(state(s)), the same f32
    subtraction: that case (nearly every candidate of a frame) asks RefBias once per string s instead of once per (s, c).
    tests/test_ctc_bias.py compares the two on random strings.  memo: a dict the caller keeps for one phrase set."""
    if 'units' not in memo:
        memo['units'] = {u for p in rb.phrases for u in p}
    if c in memo['units']:
        return float(rb.addend(s, c))
    key = s[-16:]
    v = memo.get(key)
    if v is None:
        v = memo[key] = float(F32(F32(0) - rb.psi(rb.state(key))))
    return v


def decode_one(lp, length, W, K, rb, lm=None, alpha=0.0, beta=0.0, blank=0, gaps=None, refunds=None):
    """lp [T, V], rb a tests.bias_ref.RefBias, lm None or a tests.ngram_ref.RefLM -> list of (tokens tuple, score, lm score, bias
    score) in the final order; `gaps` as in ctc_prefix_ref; `refunds` receives [(tokens, psi(state(tokens)))] in the order the last
    selection left, before the refund"""
    lm_memo, b_memo = {}, {}

    def a_lm(s, c):
        if lm is None:
            return 0.0
        key = (lm.context(s), c)
        v = lm_memo.get(key)
        if v is None:
            v = lm_memo[key] = alpha * lm.cond(key[0], c) + beta
        return v
    beam = [((), 0.0, NEG_INF)]
    lms, bss = {(): 0.0}, {(): 0.0}
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
                add_lm, add_b = a_lm(s, c), phrase_addend(rb, s, c, b_memo)
                if s2 not in lms:
                    lms[s2] = lms[s] + add_lm
                    bss[s2] = bss[s] + add_b
                e = entry(s2, (in_beam[s2], -1) if s2 in in_beam else (i, c))
                e[1] = lae(e[1], base + p + add_lm + add_b)
        scored = [(lae(pb, pnb), key, s, pb, pnb) for s, (pb, pnb, key) in new.items()]
        scored = [x for x in scored if x[0] > NEG_INF]
        scored.sort(key=lambda x: (-x[0], x[1]))
        if gaps is not None:
            gaps.append(scored[W - 1][0] - scored[W][0] if len(scored) > W else math.inf)
        beam = [(s, pb, pnb) for _, _, s, pb, pnb in scored[:W]]
        lms = {s: lms[s] for s, _, _ in beam}
        bss = {s: bss[s] for s, _, _ in beam}
        if not beam:
            break
    psi = [float(rb.psi(rb.state(s))) for s, _, _ in beam]
    if refunds is not None:
        refunds.append([(s, r) for (s, _, _), r in zip(beam, psi)])
    out = [(s, lae(pb, pnb) - r, lms[s], bss[s] - r) for (s, pb, pnb), r in zip(beam, psi)]
    out.sort(key=lambda x: -x[1])                       # stable: ties keep the last selection's order
    return out


def decode(log_probs, lengths, W, K, rb, lm=None, alpha=0.0, beta=0.0, blank=0, min_gap=None, refunds=None):
    """log_probs [B, T, V] -> tokens int64 [B, W, T] (-1 padded), out_len int32 [B, W], scores, lm_scores, bias_scores [B, W]
    (float64), laid out as the kernel's outputs; `min_gap` receives each utterance's smallest W/W+1 boundary gap, `refunds` each
    utterance's pre-refund beam (decode_one)"""
    log_probs = np.asarray(log_probs, dtype=np.float64)
    B, T, V = log_probs.shape
    K = min(K, V)
    tokens = -np.ones((B, W, T), np.int64)
    out_len = np.zeros((B, W), np.int32)
    scores = np.full((B, W), NEG_INF)
    lm_scores, bias_scores = np.zeros((B, W)), np.zeros((B, W))
    for b in range(B):
        g = []
        hyps = decode_one(log_probs[b], min(max(int(lengths[b]), 0), T), W, K, rb, lm, alpha, beta, blank, g, refunds)
        if min_gap is not None:
            min_gap.append(min(g, default=math.inf))
        for r, (s, sc, ls, bs) in enumerate(hyps):
            tokens[b, r, :len(s)] = s
            out_len[b, r] = len(s)
            scores[b, r] = sc
            lm_scores[b, r] = ls
            bias_scores[b, r] = bs
    return tokens, out_len, scores, lm_scores, bias_scores
