"""Plain numpy float64 restatement of the MWER loss (include/otrans_hip.h otr_mwer_loss): the N-best approximation of the expected
number of errors and its gradient into the logits, written for reading, with a central-difference check of its own.

B utterances with N hypothesis slots each, slot h = b * N + n.  x [B*N, max_len, >= V] logits (columns at or past V are ignored),
ys_out int [B*N, max_len] targets (-1 behind a hypothesis), n_rows int [B*N] (len + 1, 0 = dead), errors int [B, N] (< 0 = invalid)."""
import numpy as np


def _logsumexp(row):
    m = row.max()
    return m + np.log(np.exp(row - m).sum())


def forward(x, ys_out, n_rows, errors, V):
    """dict: loss, seq_logp [B, N] (-inf: not live), live bool [B, N], post [B, N], utt_err [B], c [B, N] (the gradient's per-slot
    factor P_n (W_n - E_b) / B_live), b_live"""
    x = np.asarray(x, np.float64)
    errors = np.asarray(errors)
    B, N = errors.shape
    max_len = x.shape[1]
    s = np.full((B, N), -np.inf)
    live = np.zeros((B, N), bool)
    for b in range(B):
        for n in range(N):
            h = b * N + n
            rows = min(max(int(n_rows[h]), 0), max_len)
            tg = [int(t) for t in ys_out[h][:rows]]
            if rows > 0 and errors[b, n] >= 0 and all(0 <= t < V for t in tg):
                live[b, n] = True
                s[b, n] = sum(x[h, l, t] - _logsumexp(x[h, l, :V]) for l, t in enumerate(tg))
    post = np.zeros((B, N))
    utt_err = np.zeros(B)
    for b in range(B):
        if live[b].any():
            e = np.where(live[b], np.exp(s[b] - s[b][live[b]].max()), 0.0)
            post[b] = e / e.sum()
            utt_err[b] = float((post[b] * np.where(live[b], errors[b], 0)).sum())
    b_live = int(live.any(axis=1).sum())
    loss = utt_err.sum() / b_live if b_live else 0.0
    c = post * (np.where(live, errors, 0) - utt_err[:, None]) / b_live if b_live else np.zeros((B, N))
    return {'loss': loss, 'seq_logp': s, 'live': live, 'post': post, 'utt_err': utt_err, 'c': c, 'b_live': b_live}


def grad(x, ys_out, n_rows, errors, V, g=1.0):
    """d loss / d x [B*N, max_len, V] times g: g c_h (1[v == target] - softmax(x[h, l, :V])_v) on the rows of live slots, zero elsewhere"""
    x = np.asarray(x, np.float64)
    f = forward(x, ys_out, n_rows, errors, V)
    B, N = f['c'].shape
    d = np.zeros((x.shape[0], x.shape[1], V))
    for b in range(B):
        for n in range(N):
            if not f['live'][b, n]:
                continue
            h = b * N + n
            for l in range(min(int(n_rows[h]), x.shape[1])):
                p = np.exp(x[h, l, :V] - _logsumexp(x[h, l, :V]))
                onehot = np.zeros(V)
                onehot[int(ys_out[h, l])] = 1.0
                d[h, l] = g * f['c'][b, n] * (onehot - p)
    return d


def finite_difference_error(x, ys_out, n_rows, errors, V, picks, eps=1e-5):
    """max |grad - central difference of loss| over the elements `picks` = [(h, l, v), ...]"""
    x = np.array(x, np.float64)
    d = grad(x, ys_out, n_rows, errors, V)
    worst = 0.0
    for h, l, v in picks:
        keep = x[h, l, v]
        x[h, l, v] = keep + eps
        up = forward(x, ys_out, n_rows, errors, V)['loss']
        x[h, l, v] = keep - eps
        dn = forward(x, ys_out, n_rows, errors, V)['loss']
        x[h, l, v] = keep
        worst = max(worst, abs((up - dn) / (2 * eps) - d[h, l, v]))
    return worst


def case(rng, B, N, max_len, V, rows_per_utt=(3, 9, 1, 6), scale=1.0, max_err=6):
    """the recipe of tests/test_gpu_mwer.py: unit-normal logits, all slots of an utterance share a length (utterance b:
    rows_per_utt[b % 4] rows, cut to max_len); for N >= 5 slot 1 of utterance 0 is dead and slot 2 of utterance 1 a row shorter"""
    nh = B * N
    x = rng.normal(size=(nh, max_len, V)) * scale
    n_rows = np.zeros(nh, np.int32)
    ys_out = -np.ones((nh, max_len), np.int64)
    for b in range(B):
        for n in range(N):
            r = min(rows_per_utt[b % len(rows_per_utt)], max_len)
            if N >= 5 and (b, n) == (0, 1):
                r = 0
            if N >= 5 and (b, n) == (1, 2):
                r = max(r - 1, 1)
            n_rows[b * N + n] = r
            if r:
                ys_out[b * N + n, :r - 1] = rng.integers(2, V, size=r - 1) if V > 2 else 0
                ys_out[b * N + n, r - 1] = 1 if V > 1 else 0
    errors = rng.integers(0, max_err + 1, size=(B, N)).astype(np.int32)
    return x, ys_out, n_rows, errors
