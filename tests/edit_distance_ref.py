"""Pure-Python / numpy restatement of the edit-distance scoring as include/otrans_hip.h states it (otr_edit_distance): not a test.

D[i][j] is the Levenshtein table with unit costs, i over the reference and j over the hypothesis.  The counts (S, D, I) belong to one
canonical alignment: cell (i, j) takes, among the predecessors that achieve D[i][j], the diagonal first (match or substitution), then
the cell above (deletion), then the cell to the left (insertion); row 0 is all insertions, column 0 all deletions.

    pair            the table cell by cell, carrying the counts forward
    pair_backtrace  the plain distance table first, then a walk back from (R, H) with the same preference: a second route
    pair_fast       numpy, one row at a time (the left dependence as a running minimum): for the 2048-long case
    batch           dist / counts / totals over [B, N] pairs with the validity rules
"""
import numpy as np

TOTALS = ('utterances', 'ref_tokens', 'errors_1best', 'S_1best', 'D_1best', 'I_1best', 'errors_oracle', 'bad')


def pair(ref, hyp):
    """-> (dist, S, D, I)"""
    R, H = len(ref), len(hyp)
    prev = [(j, 0, 0, j) for j in range(H + 1)]                  # row 0: j insertions
    for i in range(1, R + 1):
        cur = [(i, 0, i, 0)]                                     # column 0: i deletions
        for j in range(1, H + 1):
            dg, up, lf = prev[j - 1], prev[j], cur[j - 1]
            c = 0 if ref[i - 1] == hyp[j - 1] else 1
            best = min(dg[0] + c, up[0] + 1, lf[0] + 1)
            if dg[0] + c == best:
                cur.append((best, dg[1] + c, dg[2], dg[3]))
            elif up[0] + 1 == best:
                cur.append((best, up[1], up[2] + 1, up[3]))
            else:
                cur.append((best, lf[1], lf[2], lf[3] + 1))
        prev = cur
    return prev[H]


def pair_backtrace(ref, hyp):
    """the same (dist, S, D, I) from the plain distance table and a walk back from the corner"""
    R, H = len(ref), len(hyp)
    D = [[0] * (H + 1) for _ in range(R + 1)]
    for j in range(H + 1):
        D[0][j] = j
    for i in range(1, R + 1):
        D[i][0] = i
        for j in range(1, H + 1):
            D[i][j] = min(D[i - 1][j - 1] + (ref[i - 1] != hyp[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    i, j, s, d, ins = R, H, 0, 0, 0
    while i > 0 or j > 0:
        if i == 0:
            ins += 1
            j -= 1
        elif j == 0:
            d += 1
            i -= 1
        else:
            c = int(ref[i - 1] != hyp[j - 1])
            if D[i - 1][j - 1] + c == D[i][j]:
                s += c
                i -= 1
                j -= 1
            elif D[i - 1][j] + 1 == D[i][j]:
                d += 1
                i -= 1
            else:
                ins += 1
                j -= 1
    return (D[R][H], s, d, ins)


def pair_fast(ref, hyp):
    """numpy, row by row.  E[j] = min(diag + c, up + 1) with the diagonal winning ties; then D[i][j] = j + min_{k <= j}(E[k] - k), the
    largest such k: that cell is reached from (i, k) by j - k insertions, and a later k is a predecessor nearer in the preference."""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    R, H = len(ref), len(hyp)
    cols = np.arange(H + 1, dtype=np.int64)
    cost = cols.copy()
    cnt = np.zeros((H + 1, 3), np.int64)
    cnt[:, 2] = cols
    for i in range(1, R + 1):
        c = (hyp != ref[i - 1]).astype(np.int64)
        ed, eu = cost[:-1] + c, cost[1:] + 1
        diag = ed <= eu
        e = np.concatenate([[i], np.where(diag, ed, eu)])
        ecnt = np.empty_like(cnt)
        ecnt[0] = (0, i, 0)
        ecnt[1:] = np.where(diag[:, None], cnt[:-1] + np.stack([c, 0 * c, 0 * c], 1), cnt[1:] + np.array([0, 1, 0]))
        key = e - cols
        run = np.minimum.accumulate(key)
        k = np.maximum.accumulate(np.where(key == run, cols, 0))    # the largest k <= j with key[k] == min_{k' <= j} key[k']
        cost = run + cols
        cnt = ecnt[k]
        cnt[:, 2] += cols - k
    return (int(cost[H]), int(cnt[H, 0]), int(cnt[H, 1]), int(cnt[H, 2]))


def batch(ref, ref_len, hyp, hyp_len=None, eos=-1, fn=pair):
    """ref [B, Lr], ref_len [B], hyp [B, N, Lh] (or [B, Lh]), hyp_len [B, N] (None: the full width).  -> dist int32 [B, N], counts int32
    [B, N, 3], totals int64 [8] (of this call alone), as the header defines them."""
    ref, hyp = np.asarray(ref), np.asarray(hyp)
    if hyp.ndim == 2:
        hyp = hyp[:, None]
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    hyp_len = np.full((B, N), Lh) if hyp_len is None else np.asarray(hyp_len).reshape(B, N)
    dist = np.full((B, N), -1, np.int32)
    counts = np.full((B, N, 3), -1, np.int32)
    totals = np.zeros(8, np.int64)
    for b in range(B):
        R = int(ref_len[b])
        ref_ok = 0 <= R <= Lr
        for n in range(N):
            H = int(hyp_len[b, n])
            if not ref_ok or not 0 <= H <= Lh:
                continue
            h = [int(t) for t in hyp[b, n, :H]]
            if eos >= 0 and eos in h:
                h = h[:h.index(eos)]
            r = fn([int(t) for t in ref[b, :R]], h)
            dist[b, n] = r[0]
            counts[b, n] = r[1:]
        if dist[b, 0] < 0:
            totals[7] += 1
            continue
        totals[0] += 1
        totals[1] += R
        totals[2] += dist[b, 0]
        totals[3:6] += counts[b, 0]
        totals[6] += min(int(d) for d in dist[b] if d >= 0)
    return dist, counts, totals
