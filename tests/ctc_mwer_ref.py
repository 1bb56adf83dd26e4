"""Plain numpy float64 restatement of the MWER loss of the CTC model (include/otrans_hip.h otr_ctc_mwer_loss): the N-best expected number
of errors under the CTC likelihoods of the hypotheses, the interpolated CTC loss on the reference, and the gradient into the LOGITS
(the log-softmax included), written for reading, with its own alpha / beta recursion and a central-difference check of its own.

logits [B, T, V]; in_len [B] (clamped to [0, T]); hyps int [B, N, L] (anything behind a length is never looked at), hyp_len [B, N],
errors int [B, N] (< 0: invalid); ref int [B, W] with ref_len [B], or None."""
import numpy as np

NEG = -np.inf


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def ctc_occupancy(lp, labels, blank):
    """CTC of log-probs lp [Tb, V] against `labels`: (ll, gamma [Tb, V]) with gamma[t, v] the posterior probability that frame t emits v
    (its rows sum to 1); (-inf, None) if no alignment exists.  Extended states 0 .. 2L: blank, l_1, blank, ..., l_L, blank."""
    Tb, L = lp.shape[0], len(labels)
    if Tb == 0:
        return NEG, None
    ext = np.full(2 * L + 1, blank, np.int64)
    ext[1::2] = labels
    S = len(ext)
    skip = np.zeros(S, bool)                                   # s - 2 -> s allowed
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    alpha = np.full((Tb, S), NEG)
    alpha[0, 0] = lp[0, blank]
    if S > 1:
        alpha[0, 1] = lp[0, ext[1]]
    for t in range(1, Tb):
        a = alpha[t - 1].copy()
        a[1:] = np.logaddexp(a[1:], alpha[t - 1, :-1])
        a[2:] = np.where(skip[2:], np.logaddexp(a[2:], alpha[t - 1, :-2]), a[2:])
        alpha[t] = a + lp[t, ext]
    ll = np.logaddexp(alpha[-1, -1], alpha[-1, -2]) if S > 1 else alpha[-1, -1]
    if ll == NEG:
        return NEG, None
    beta = np.full((Tb, S), NEG)                               # beta_t(s) includes the emission at t, as alpha does
    beta[-1, -1] = lp[-1, ext[-1]]
    if S > 1:
        beta[-1, -2] = lp[-1, ext[-2]]
    for t in range(Tb - 2, -1, -1):
        b = beta[t + 1].copy()
        b[:-1] = np.logaddexp(b[:-1], beta[t + 1, 1:])
        b[:-2] = np.where(skip[2:], np.logaddexp(b[:-2], beta[t + 1, 2:]), b[:-2])
        beta[t] = b + lp[t, ext]
    gamma = np.zeros_like(lp)
    with np.errstate(invalid='ignore'):
        occ = np.exp(alpha + beta - lp[:, ext] - ll)           # [Tb, S]; -inf + -inf - ... = -inf or nan where lp is -inf
    occ = np.nan_to_num(occ, nan=0.0)
    for s in range(S):
        gamma[:, ext[s]] += occ[:, s]
    return ll, gamma


def _bound(hyps, ref, max_tgt):
    if max_tgt is not None:
        return max_tgt
    return min(max(hyps.shape[2], ref.shape[1] if ref is not None else 0), 127)


def forward(logits, in_len, hyps, hyp_len, errors, ref=None, ref_len=None, ctc_weight=0.0, scale=1.0, blank=0, max_tgt=None):
    """dict: loss, mwer, ctc, seq_logp [B, N] (-inf: not live), live bool [B, N], post [B, N], utt_err [B], nll_ref [B], ok_ref bool
    [B], coef_ref [B], c [B, N] (the gradient's per-slot factor scale * P_n (W_n - E_b) / B_live), b_live, and the occupancies
    gamma[(b, n)] / gamma_ref[b] of the live slots / feasible references"""
    x = np.asarray(logits, np.float64)
    B, T, V = x.shape
    errors = np.asarray(errors)
    N = errors.shape[1]
    mt = _bound(np.asarray(hyps), ref, max_tgt)
    lp = log_softmax(x)
    Tb = np.clip(np.asarray(in_len), 0, T)
    s = np.full((B, N), NEG)
    live = np.zeros((B, N), bool)
    gamma, gamma_ref = {}, {}
    for b in range(B):
        for n in range(N):
            L = int(hyp_len[b][n])
            if errors[b, n] < 0 or not 0 <= L <= mt:
                continue
            lab = [int(t) for t in hyps[b][n][:L]]
            if not all(0 <= t < V for t in lab):
                continue
            ll, gm = ctc_occupancy(lp[b, :Tb[b]], lab, blank)
            if ll > NEG:
                live[b, n], s[b, n], gamma[(b, n)] = True, ll, gm
    post = np.zeros((B, N))
    utt_err = np.zeros(B)
    for b in range(B):
        if live[b].any():
            e = np.where(live[b], np.exp(scale * s[b] - (scale * s[b][live[b]]).max()), 0.0)
            post[b] = e / e.sum()
            utt_err[b] = float((post[b] * np.where(live[b], errors[b], 0)).sum())
    b_live = int(live.any(axis=1).sum())
    mwer = utt_err.sum() / b_live if b_live else 0.0
    c = scale * post * (np.where(live, errors, 0) - utt_err[:, None]) / b_live if b_live else np.zeros((B, N))
    nll_ref, ok_ref, coef_ref = np.zeros(B), np.zeros(B, bool), np.zeros(B)
    if ref is not None:
        for b in range(B):
            L = int(ref_len[b])
            good = 0 <= L <= mt
            coef_ref[b] = 1.0 / (B * max(L if good else 0, 1))
            lab = [int(t) for t in ref[b][:L]] if good else []
            if good and all(0 <= t < V for t in lab):
                ll, gm = ctc_occupancy(lp[b, :Tb[b]], lab, blank)
                if ll > NEG:
                    ok_ref[b], nll_ref[b], gamma_ref[b] = True, -ll, gm
    ctc = float((nll_ref * coef_ref).sum())
    return {'loss': mwer + ctc_weight * ctc, 'mwer': mwer, 'ctc': ctc, 'seq_logp': s, 'live': live, 'post': post, 'utt_err': utt_err,
            'nll_ref': nll_ref, 'ok_ref': ok_ref, 'coef_ref': coef_ref, 'c': c, 'b_live': b_live, 'gamma': gamma, 'gamma_ref': gamma_ref,
            'lp': lp, 'Tb': Tb}


def grad(logits, in_len, hyps, hyp_len, errors, ref=None, ref_len=None, ctc_weight=0.0, scale=1.0, blank=0, max_tgt=None, g=1.0,
         parts=False):
    """d loss / d logits [B, T, V] times g, in the form the kernel uses: the hypotheses' softmax terms cancel (sum_n c_n = 0), so
    the MWER part is sum_n c_n gamma_n alone; the CTC part is ctc_weight * coef_b * (softmax - gamma_ref) on the frames below in_len.
    parts: (mwer part, ctc part) instead of their sum."""
    f = forward(logits, in_len, hyps, hyp_len, errors, ref, ref_len, ctc_weight, scale, blank, max_tgt)
    B, T, V = f['lp'].shape
    dm, dc = np.zeros((B, T, V)), np.zeros((B, T, V))
    for (b, n), gm in f['gamma'].items():
        dm[b, :f['Tb'][b]] += g * f['c'][b, n] * gm
    for b, gm in f['gamma_ref'].items():
        dc[b, :f['Tb'][b]] = g * ctc_weight * f['coef_ref'][b] * (np.exp(f['lp'][b, :f['Tb'][b]]) - gm)
    return (dm, dc) if parts else dm + dc


def finite_difference_error(picks, logits, *args, eps=1e-5, **kw):
    """max |grad - central difference of loss| over the elements `picks` = [(b, t, v), ...]"""
    x = np.array(logits, np.float64)
    d = grad(x, *args, **kw)
    worst = 0.0
    for b, t, v in picks:
        keep = x[b, t, v]
        x[b, t, v] = keep + eps
        up = forward(x, *args, **kw)['loss']
        x[b, t, v] = keep - eps
        dn = forward(x, *args, **kw)['loss']
        x[b, t, v] = keep
        worst = max(worst, abs((up - dn) / (2 * eps) - d[b, t, v]))
    return worst
