"""Plain numpy restatement of CTC segmentation as include/otrans_hip.h states it (otr_ctc_segment), in np.float32, one frame of all
states at a time: not a test.

Extended states s = 0 .. 2L (even: blank, odd: label s >> 1), x_t(c) the log-prob of token c at frame t, T_b frames, skip_logp <= 0:
    v_0(0) = x_0(blank), v_0(1) = x_0(label 0), -inf elsewhere; both carry code 3 ("the path starts here")
    t >= 1: candidates in tie order: stay v_{t-1}(s) [code 0]; v_{t-1}(s-1) [1]; v_{t-1}(s-2) if ext(s) is a label and differs from
    ext(s-2) [2]; for s in {0, 1} and only with free_start the virtual start float32(t) * skip_logp [3].  A later candidate wins only
    if strictly greater.  v_t(s) = max + x_t(ext(s)), one float32 add.
    end: with free_end every frame t, for s = 2L and then 2L-1: e = v_t(s) + tail, tail = float32(T_b-1-t) * skip_logp for t < T_b-1
    and exactly 0 at the last frame; otherwise t = T_b-1 alone.  The largest e wins, on ties the earliest t, then 2L before 2L-1.
The trace follows the codes back until it meets a 3.  Outputs as the kernel's: frame_token (token on covered frames, blank on blank
frames, -1 on skipped frames and past T_b), spans, label_logp (ascending t), score, bounds (first covered frame, one past the last).
Infeasible (L < 1, L > max_tgt, a label outside [0, V), T_b = 0, no finite path): score -inf, frame_token / spans / bounds -1,
label_logp 0.  confidence() restates segment.CTCSegmenter's utterance confidence in float64."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def segment_one(lp, length, labels, blank=0, free_start=True, free_end=True, skip_logp=0.0):
    """lp [T, V] float32, `length` >= 1 frames of it used, labels: list of >= 1 ints in [0, V).  Returns (score float32, first frame,
    states: the extended states of frames first .. first + len(states) - 1) or (-inf, -1, None) when no path of finite score exists."""
    lp = np.asarray(lp, dtype=np.float32)
    skip_logp = np.float32(skip_logp)
    L = len(labels)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = (ext[3::2] != blank) & (ext[3::2] != ext[1:-2:2])
    v = np.full(S, NEG_INF, np.float32)
    v[0], v[1] = lp[0, blank], lp[0, ext[1]]
    back = np.zeros((length, S), np.int8)
    back[0, :2] = 3
    best, best_t, best_s = NEG_INF, -1, -1

    def consider(t, v, best, best_t, best_s):
        tail = np.float32(np.float32(length - 1 - t) * skip_logp) if t < length - 1 else np.float32(0.0)
        for s in (2 * L, 2 * L - 1):
            e = np.float32(v[s] + tail)
            if e > best:
                best, best_t, best_s = e, t, s
        return best, best_t, best_s

    with np.errstate(invalid='ignore'):
        for t in range(1, length):
            if free_end:
                best, best_t, best_s = consider(t - 1, v, best, best_t, best_s)
            m, k = v.copy(), back[t]
            a1 = np.empty(S, np.float32)
            a1[0], a1[1:] = NEG_INF, v[:-1]
            sel = a1 > m
            m[sel], k[sel] = a1[sel], 1
            a2 = np.full(S, NEG_INF, np.float32)
            a2[2:] = v[:-2]
            sel = skip & (a2 > m)
            m[sel], k[sel] = a2[sel], 2
            if free_start:
                vs = np.float32(np.float32(t) * skip_logp)         # one float32 multiply of the exactly converted t
                for s in (0, 1):
                    if vs > m[s]:
                        m[s], k[s] = vs, 3
            v = (m + lp[t, ext]).astype(np.float32)                # float32 + float32: one correctly rounded add
        best, best_t, best_s = consider(length - 1, v, best, best_t, best_s)
    if not best > NEG_INF:
        return NEG_INF, -1, None
    states, s, t = [], best_s, best_t
    while True:
        states.append(s)
        code = int(back[t, s])
        if code == 3:
            break
        s -= code
        t -= 1
    return best, t, states[::-1]


def segment(log_probs, in_len, targets, tgt_len, blank=0, free_start=True, free_end=True, skip_logp=0.0):
    """log_probs [B, T, V], in_len [B], targets [B, max_tgt], tgt_len [B] -> (frame_token int32 [B, T], spans int32 [B, max_tgt, 2],
    label_logp float32 [B, max_tgt], score float32 [B], bounds int32 [B, 2]) laid out as the kernel's outputs"""
    log_probs = np.asarray(log_probs, dtype=np.float32)
    targets = np.asarray(targets)
    B, T, V = log_probs.shape
    max_tgt = targets.shape[1]
    frame_token = -np.ones((B, T), np.int32)
    spans = -np.ones((B, max_tgt, 2), np.int32)
    label_logp = np.zeros((B, max_tgt), np.float32)
    score = np.full((B,), NEG_INF, np.float32)
    bounds = -np.ones((B, 2), np.int32)
    for b in range(B):
        L, n = int(tgt_len[b]), min(max(int(in_len[b]), 0), T)
        if L < 1 or L > max_tgt or n == 0:
            continue
        labels = [int(c) for c in targets[b, :L]]
        if any(c < 0 or c >= V for c in labels):
            continue
        sc, first, states = segment_one(log_probs[b], n, labels, blank, free_start, free_end, skip_logp)
        if states is None:
            continue
        score[b] = sc
        st = np.asarray(states)
        end = first + len(states)
        bounds[b] = (first, end)
        lab = np.asarray(labels + [blank])                         # the final blank's st >> 1 is L: np.where indexes it too
        frame_token[b, first:end] = np.where(st & 1, lab[st >> 1], blank)
        for j in range(L):
            ts = first + np.nonzero(st == 2 * j + 1)[0]
            spans[b, j] = (ts[0], ts[-1] + 1)
            acc = np.float32(0.0)
            for x in log_probs[b, ts[0]:ts[-1] + 1, labels[j]]:
                acc = np.float32(acc + x)
            label_logp[b, j] = acc
    return frame_token, spans, label_logp, score, bounds


def confidence(label_logp, spans, lengths, conf_window=8):
    """The utterance confidences in float64: the labels of one recording are the utterances of `lengths` labels each, one after the
    other.  m_j = label_logp_j / (end_j - start_j); per utterance the minimum, over every window of w = min(conf_window, n_u)
    consecutive labels of it, of the mean of m_j."""
    llp = np.asarray(label_logp, dtype=np.float64)
    sp = np.asarray(spans, dtype=np.float64)
    out, at = [], 0
    for n in lengths:
        m = llp[at:at + n] / (sp[at:at + n, 1] - sp[at:at + n, 0])
        w = min(conf_window, n)
        out.append(min(float(m[a:a + w].mean()) for a in range(n - w + 1)))
        at += n
    return out
