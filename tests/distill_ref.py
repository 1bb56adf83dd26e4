"""Plain numpy restatement of the knowledge-distillation loss (include/otrans_hip.h otr_distill_loss), dense and sparse, written for
reading, in a chosen dtype: float64 is the reference, float32 the yardstick for what fp32 rounding alone does to the same numbers.

Rows are [B, T]; row (b, i) is live iff i < min(max(lengths[b], 0), T) (and, sparse, it lists an entry; dense, its teacher row holds
an element above -inf).  student / teacher [B, T, >= V] (columns at or past V are ignored), top_val / top_idx [B, T, K]."""
import numpy as np


def _log_softmax(x):
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def live_rows(lengths, B, T):
    n = np.clip(np.asarray(lengths).astype(np.int64), 0, T)
    return np.arange(T)[None, :] < n[:, None]


def _row(s, q_logits, tau, dtype):
    """one row: student logits s [V] and the teacher's logits q_logits [V] (-inf: no mass) -> (kl, p, q), or None without teacher mass"""
    with np.errstate(divide='ignore', invalid='ignore'):
        if not np.isfinite(q_logits).any():
            return None
        tau = dtype(tau)
        lp = _log_softmax(s.astype(dtype) / tau)
        has = q_logits > -np.inf
        lq = np.full(s.shape, -np.inf, dtype)
        lq[has] = _log_softmax(q_logits[has].astype(dtype) / tau)
        q = np.exp(lq)
        kl = (q[has] * (lq[has] - lp[has])).sum(dtype=dtype)
    return kl, np.exp(lp), q


def forward(student, lengths, V, tau, teacher=None, top_val=None, top_idx=None, g=1.0, dtype=np.float64):
    """dict: loss, row_kl [B, T], live bool [B, T], n_live, p and q [B, T, V] (0 on dead rows), grad [B, T, V] = g tau / n_live (p - q)"""
    B, T = student.shape[:2]
    live = live_rows(lengths, B, T)
    row_kl = np.zeros((B, T), dtype)
    p = np.zeros((B, T, V), dtype)
    q = np.zeros((B, T, V), dtype)
    for b in range(B):
        for i in range(T):
            if not live[b, i]:
                continue
            if teacher is not None:
                ql = np.asarray(teacher[b, i, :V])
            else:
                ql = np.full(V, -np.inf, top_val.dtype)
                idx = np.asarray(top_idx[b, i]).astype(np.int64)
                ok = (idx >= 0) & (idx < V)
                assert len(set(idx[ok].tolist())) == int(ok.sum()), 'indices within a row must be distinct'
                listed = np.zeros(V, bool)
                listed[idx[ok]] = True
                ql[idx[ok]] = top_val[b, i][ok]
                if not listed.any():
                    live[b, i] = False
                    continue
            r = _row(np.asarray(student[b, i, :V]), ql, tau, dtype)
            if r is None:
                live[b, i] = False
                continue
            row_kl[b, i], p[b, i], q[b, i] = r
    n_live = int(live.sum())
    tau_d = dtype(tau)
    loss = tau_d * tau_d * row_kl.sum(dtype=dtype) / dtype(n_live) if n_live else dtype(0)
    grad = dtype(g) * tau_d / dtype(n_live) * (p - q) if n_live else np.zeros((B, T, V), dtype)
    return {'loss': loss, 'row_kl': row_kl, 'live': live, 'n_live': n_live, 'p': p, 'q': q, 'grad': grad}


def case(rng, B, T, V, pad_s=0, pad_t=0):
    """the recipe of tests/test_gpu_distill.py: student ~ N(0, 4^2), teacher = student + N(0, 2^2), as f32 [B, T, V + pad] whose pad
    columns hold random numbers that must not matter"""
    s = rng.normal(size=(B, T, V + pad_s)) * 4.0
    t = rng.normal(size=(B, T, V + pad_t)) * 4.0
    t[:, :, :V] = s[:, :, :V] + rng.normal(size=(B, T, V)) * 2.0
    return s.astype(np.float32), t.astype(np.float32)


def topk(x, K):
    """(val [.., K] descending, idx int32 [.., K], ties to the lower index) of the last axis"""
    order = np.argsort(-x, axis=-1, kind='stable')[..., :K]
    return np.take_along_axis(x, order, axis=-1), order.astype(np.int32)
