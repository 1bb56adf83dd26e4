"""Pure-Python / numpy restatement of the per-token alignment and the n-best consensus as include/otrans_hip.h states them
(otr_edit_align, otr_nbest_consensus): not a test.  Everything that is not an integer is float64.

    align           the plain distance table, then the walk back from (R, H): diagonal, then above, then left
    align_batch     dist / code / ref_pos over [B, N] pairs with the validity rules of edit_distance_ref.batch
    consensus       post / risk / best / conf of an n-best
    calibration     NCE and ECE (10 equal-width bins) of confidences against 0 / 1 outcomes, as evaluate.calibration defines them
"""
import math

import numpy as np

MATCH, SUB, INS = 0, 1, 2


def align(ref, hyp):
    """-> (dist, code [H], ref_pos [H]): per hypothesis token 0 match / 1 substitution / 2 insertion, and the index of the reference
    token it is aligned to (-1 on insertions)"""
    R, H = len(ref), len(hyp)
    D = np.zeros((R + 1, H + 1), np.int64)
    D[0, :] = np.arange(H + 1)
    D[:, 0] = np.arange(R + 1)
    hy = np.asarray(hyp, np.int64).reshape(H)
    for i in range(1, R + 1):
        e = np.minimum(D[i - 1, :-1] + (hy != ref[i - 1]), D[i - 1, 1:] + 1)      # diagonal or above
        key = np.concatenate([[i], e]) - np.arange(H + 1)
        D[i] = np.minimum.accumulate(key) + np.arange(H + 1)                      # ... or any run of insertions behind one of them
    code, pos = [-1] * H, [-1] * H
    i, j = R, H
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
            code[j] = INS
        elif j == 0:
            i -= 1
        else:
            c = int(ref[i - 1] != hyp[j - 1])
            if D[i - 1, j - 1] + c == D[i, j]:
                i -= 1
                j -= 1
                code[j], pos[j] = (SUB if c else MATCH), i
            elif D[i - 1, j] + 1 == D[i, j]:
                i -= 1
            else:
                j -= 1
                code[j] = INS
    return int(D[R, H]), code, pos


def _cut(tokens, n, eos):
    h = [int(t) for t in tokens[:n]]
    if eos >= 0 and eos in h:
        h = h[:h.index(eos)]
    return h


def align_batch(ref, ref_len, hyp, hyp_len=None, eos=-1):
    """ref [B, Lr], ref_len [B], hyp [B, N, Lh] (or [B, Lh]), hyp_len [B, N] (None: the full width) -> dist int32 [B, N], code int8
    [B, N, Lh], ref_pos int32 [B, N, Lh]; -1 past a hypothesis's end and for an invalid pair"""
    ref, hyp = np.asarray(ref), np.asarray(hyp)
    if hyp.ndim == 2:
        hyp = hyp[:, None]
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    hyp_len = np.full((B, N), Lh) if hyp_len is None else np.asarray(hyp_len).reshape(B, N)
    dist = np.full((B, N), -1, np.int32)
    code = np.full((B, N, Lh), -1, np.int8)
    pos = np.full((B, N, Lh), -1, np.int32)
    for b in range(B):
        R = int(ref_len[b])
        for n in range(N):
            H = int(hyp_len[b, n])
            if not 0 <= R <= Lr or not 0 <= H <= Lh:
                continue
            h = _cut(hyp[b, n], H, eos)
            d, c, p = align([int(t) for t in ref[b, :R]], h)
            dist[b, n] = d
            code[b, n, :len(h)] = c
            pos[b, n, :len(h)] = p
    return dist, code, pos


def consensus(tokens, lengths=None, scores=None, scale=1.0, eos=-1):
    """tokens [B, N, L], lengths [B, N] (None: the full width), scores [B, N] (None: zeros) -> post f64 [B, N], risk f64 [B, N], best
    int32 [B], conf f64 [B, N, L], live bool [B, N]"""
    tokens = np.asarray(tokens)
    B, N, L = tokens.shape
    lengths = np.full((B, N), L) if lengths is None else np.asarray(lengths).reshape(B, N)
    scores = np.zeros((B, N)) if scores is None else np.asarray(scores, np.float64).reshape(B, N)
    live = np.isfinite(scores) & (lengths >= 0) & (lengths <= L)
    post = np.zeros((B, N))
    risk = np.full((B, N), np.inf)
    conf = np.zeros((B, N, L))
    best = np.full(B, -1, np.int32)
    for b in range(B):
        idx = [n for n in range(N) if live[b, n]]
        if not idx:
            continue
        x = np.array([scale * scores[b, n] for n in idx])
        e = np.exp(x - x.max())
        post[b, idx] = e / e.sum()
        hyps = {n: _cut(tokens[b, n], int(lengths[b, n]), eos) for n in idx}
        for i in idx:
            r = 0.0
            for j in idx:                                           # ascending
                d, code, _ = align(hyps[j], hyps[i])                # hypothesis i against hypothesis j as the reference
                r += post[b, j] * d
                for k, c in enumerate(code):
                    if c == MATCH:
                        conf[b, i, k] += post[b, j]
            risk[b, i] = r
        best[b] = min(idx, key=lambda n: (risk[b, n], -scores[b, n], n))
    return post, risk, best, conf, live


def calibration(conf, correct, eps=1e-6, bins=10):
    """conf in [0, 1], correct 0 / 1 -> (nce, ece).  NCE = (H_prior - H_conf) / H_prior with H_prior the entropy of the outcomes at their
    mean rate and H_conf the cross-entropy of the confidences (clamped to [eps, 1 - eps]); nan where every outcome is the same.  ECE =
    sum over the bins [k / bins, (k + 1) / bins) (the last closed) of n_k / n * |mean outcome - mean confidence|."""
    conf = [float(c) for c in conf]
    correct = [int(c) for c in correct]
    n, nc = len(conf), sum(correct)
    if n == 0:
        return float('nan'), float('nan')
    hc = -sum(math.log(min(max(c, eps), 1 - eps)) if y else math.log(1 - min(max(c, eps), 1 - eps)) for c, y in zip(conf, correct))
    p = nc / n
    hp = -(nc * math.log(p) + (n - nc) * math.log(1 - p)) if 0 < nc < n else 0.0
    nce = (hp - hc) / hp if hp > 0 else float('nan')
    ece = 0.0
    for k in range(bins):
        sel = [(c, y) for c, y in zip(conf, correct) if min(int(c * bins), bins - 1) == k]
        if sel:
            ece += abs(sum(y for _, y in sel) - sum(c for c, _ in sel)) / n
    return nce, ece
