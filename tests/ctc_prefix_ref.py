"""Plain-Python restatement of the CTC prefix beam search of include/otrans_hip.h (otr_ctc_topk + otr_ctc_beam_search), in float64.

Same semantics and the same tie order as the kernels, written from the algorithm: at each frame the candidates are the K tokens of
highest log-prob (ties -> lower token); every beam prefix s in slot i with last token l carries (pb, pnb); a candidate c with
log-prob p gives
    c == blank:  pb'(s)   = lae(pb'(s),   lae(pb(s), pnb(s)) + p)
    c == l:      pnb'(s)  = lae(pnb'(s),  pnb(s) + p);   pnb'(s+c) = lae(pnb'(s+c), pb(s) + p)
    other c:     pnb'(s+c) = lae(pnb'(s+c), lae(pb(s), pnb(s)) + p)
Equal strings merge.  The new beam is the W strings of highest lae(pb', pnb') above -inf, ties to the lower (parent slot, token),
a string already in the beam (slot i) counting as (i, -1).  No score-threshold pruning."""
import math

import numpy as np

NEG_INF = -math.inf


def lae(a, b):
    m = max(a, b)
    if m == NEG_INF:
        return NEG_INF
    return m + math.log1p(math.exp(min(a, b) - m))


def topk(row, K):
    """the K (log-prob, token) of highest log-prob, descending, ties -> lower token"""
    row = np.asarray(row, dtype=np.float64)
    order = np.lexsort((np.arange(len(row)), -row))[:K]
    return [(float(row[v]), int(v)) for v in order]


def decode_one(lp, length, W, K, blank=0, gaps=None):
    """lp [T, V] -> list of (tokens tuple, score) in beam order (descending score).  `gaps`: a list that receives, per frame, the
    score gap between the W-th and the (W+1)-th candidate (inf when there are at most W): where it is tiny, float32 rounding may
    legitimately change which prefixes survive."""
    beam = [((), 0.0, NEG_INF)]                        # slot order: (string, pb, pnb)
    for t in range(length):
        cands = topk(lp[t], K)
        new = {}                                       # string -> [pb', pnb', key]

        def entry(s, key):
            e = new.get(s)
            if e is None:
                e = new[s] = [NEG_INF, NEG_INF, key]
            return e
        in_beam = {s: i for i, (s, _, _) in enumerate(beam)}
        for i, (s, pb, pnb) in enumerate(beam):        # a string in the beam keeps its own slot's key, whoever reaches it
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
                e = entry(s2, (in_beam[s2], -1) if s2 in in_beam else (i, c))
                e[1] = lae(e[1], base + p)
        scored = [(lae(pb, pnb), key, s, pb, pnb) for s, (pb, pnb, key) in new.items()]
        scored = [x for x in scored if x[0] > NEG_INF]
        scored.sort(key=lambda x: (-x[0], x[1]))
        if gaps is not None:
            gaps.append(scored[W - 1][0] - scored[W][0] if len(scored) > W else math.inf)
        beam = [(s, pb, pnb) for _, _, s, pb, pnb in scored[:W]]
        if not beam:
            break
    return [(s, lae(pb, pnb)) for s, pb, pnb in beam]


def decode(log_probs, lengths, W, K, blank=0, min_gap=None):
    """log_probs [B, T, V], lengths [B] -> tokens int64 [B, W, T] (-1 padded), out_len int32 [B, W], scores [B, W] (float64)
    laid out as the kernel's outputs.  `min_gap`: a list that receives each utterance's smallest W/W+1 boundary gap."""
    log_probs = np.asarray(log_probs, dtype=np.float64)
    B, T, V = log_probs.shape
    K = min(K, V)
    tokens = -np.ones((B, W, T), np.int64)
    out_len = np.zeros((B, W), np.int32)
    scores = np.full((B, W), NEG_INF)
    for b in range(B):
        g = []
        hyps = decode_one(log_probs[b], min(max(int(lengths[b]), 0), T), W, K, blank, g)
        if min_gap is not None:
            min_gap.append(min(g, default=math.inf))
        for r, (s, sc) in enumerate(hyps):
            tokens[b, r, :len(s)] = s
            out_len[b, r] = len(s)
            scores[b, r] = sc
    return tokens, out_len, scores
