"""Plain numpy restatement of CTC forced alignment as include/otrans_hip.h states it (otr_ctc_align), in np.float32: not a test.

Extended states s = 0 .. 2L (even: blank, odd: label s >> 1), x_t(c) the log-prob of token c at frame t:
    v_0(0) = x_0(blank), v_0(1) = x_0(label 0), -inf elsewhere
    v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if ext(s) is a label and differs from ext(s-2)) + x_t(ext(s))
one float32 add after an exact max.  Ties: among equal predecessors the smallest step wins (stay, then s-1, then s-2); at the end
v(2L) wins a tie against v(2L-1).  Outputs as the kernel's: frame_token (blank on blank frames, -1 past the length), spans (first
frame, one-past-last frame of each label; -1 past L), label_logp (the label's log-probs over its span, added in ascending t, float32;
0 past L), score.  Infeasible (score -inf, or a length outside [0, max_tgt], or a label outside [0, V)): score -inf, frame_token and
spans -1, label_logp 0.  No frames and no labels: score 0, the empty path."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def align_one(lp, length, labels, blank=0):
    """lp [T, V] float32, `length` frames of it used, labels: list of ints.  Returns (score float32, states list of `length` extended
    states) or (-inf, None) when no path exists."""
    lp = np.asarray(lp, dtype=np.float32)
    L = len(labels)
    S = 2 * L + 1
    if length == 0:
        return (np.float32(0.0), []) if L == 0 else (NEG_INF, None)
    ext = np.array([blank if s % 2 == 0 else int(labels[s >> 1]) for s in range(S)])
    skip = np.array([s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(S)])
    x = lp[:length][:, ext]                                  # [length, S]: x_t(ext(s))
    v = np.full(S, NEG_INF, np.float32)
    v[0] = x[0, 0]
    if S > 1:
        v[1] = x[0, 1]
    back = np.zeros((length, S), np.int8)
    for t in range(1, length):                               # every state of a frame at once; the order of the two tests is the tie rule
        a1 = np.concatenate(([NEG_INF], v[:-1])).astype(np.float32)
        a2 = np.where(skip, np.concatenate(([NEG_INF, NEG_INF], v[:-2]))[:S], NEG_INF).astype(np.float32)
        m, k = v.copy(), np.zeros(S, np.int8)
        sel = a1 > m
        m[sel], k[sel] = a1[sel], 1
        sel = a2 > m
        m[sel], k[sel] = a2[sel], 2
        v = (m + x[t]).astype(np.float32)                    # float32 + float32: one correctly rounded add
        back[t] = k
    end, best = S - 1, v[S - 1]
    if S > 1 and v[S - 2] > best:
        end, best = S - 2, v[S - 2]
    if not best > NEG_INF:
        return NEG_INF, None
    states = [0] * length
    s = end
    for t in range(length - 1, 0, -1):
        states[t] = s
        s -= int(back[t, s])
    states[0] = s
    return best, states


def align(log_probs, in_len, targets, tgt_len, blank=0):
    """log_probs [B, T, V], in_len [B], targets [B, max_tgt], tgt_len [B] -> (frame_token int32 [B, T], spans int32 [B, max_tgt, 2],
    label_logp float32 [B, max_tgt], score float32 [B]) laid out as the kernel's outputs"""
    log_probs = np.asarray(log_probs, dtype=np.float32)
    targets = np.asarray(targets)
    B, T, V = log_probs.shape
    max_tgt = targets.shape[1]
    frame_token = -np.ones((B, T), np.int32)
    spans = -np.ones((B, max_tgt, 2), np.int32)
    label_logp = np.zeros((B, max_tgt), np.float32)
    score = np.full((B,), NEG_INF, np.float32)
    for b in range(B):
        L, n = int(tgt_len[b]), min(max(int(in_len[b]), 0), T)
        if L < 0 or L > max_tgt:
            continue
        labels = [int(c) for c in targets[b, :L]]
        if any(c < 0 or c >= V for c in labels):
            continue
        sc, states = align_one(log_probs[b], n, labels, blank)
        score[b] = sc
        if states is None:
            continue
        for t, s in enumerate(states):
            frame_token[b, t] = labels[s >> 1] if s & 1 else blank
        for j in range(L):
            ts = [t for t, s in enumerate(states) if s == 2 * j + 1]
            spans[b, j] = (ts[0], ts[-1] + 1)
            acc = np.float32(0.0)
            for t in ts:
                acc = np.float32(acc + log_probs[b, t, labels[j]])
            label_logp[b, j] = acc
    return frame_token, spans, label_logp, score
