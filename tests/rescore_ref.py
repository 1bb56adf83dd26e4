"""Plain-Python restatement of the attention rescoring of the CTC n-best (include/otrans_hip.h otr_rescore_pack / _score / _select;
SpeechToTextRecognizer rescore=True), in float64.

The first pass is the CTC prefix beam search (tests/ctc_prefix_ref.py): per utterance W slots in descending CTC score, each a token
tuple with the beam's score, dead slots with score -inf.  A slot is rescorable when its score is above -inf and len(h) + 1 <= max_len.
    att(h)   = sum_{l=0..len(h)} log_softmax(decoder([BOS] + h))[l, (h + [EOS])[l]]
    lm(h)    = the same sum over the LM's logits on [BOS] + h
    total(h) = (1 - lam) att(h) + lam ctc(h) + mu lm(h),  divided by ((lamda + len(h)) / (lamda + 1)) ** penalty when penalty != 0
Not rescorable: total = -inf.  Order: total descending, ties -> lower CTC rank; -inf last, in CTC order.  BOS = EOS = 1."""
import math

import numpy as np

NEG_INF = -math.inf
BOS = EOS = 1


def pack(tokens, out_len, scores, max_len, V, bos=BOS, eos=EOS):
    """tokens int64 [B, W, T] (-1 padded), out_len [B, W], scores [B, W] -> ys_in, ys_out int64 [B*W, max_len], n_rows int32 [B*W]"""
    tokens, out_len, scores = np.asarray(tokens), np.asarray(out_len), np.asarray(scores, dtype=np.float64)
    B, W, T = tokens.shape
    ys_in = np.full((B * W, max_len), eos, np.int64)
    ys_out = np.full((B * W, max_len), -1, np.int64)
    n_rows = np.zeros(B * W, np.int32)
    ys_in[:, 0] = bos
    for h in range(B * W):
        b, w = divmod(h, W)
        n = int(out_len[b, w])
        if not (scores[b, w] > NEG_INF and 0 <= n <= T and n + 1 <= max_len):
            continue
        tok = tokens[b, w, :n]
        ys_in[h, 1:1 + n] = np.clip(tok, 0, V - 1)
        ys_out[h, :n] = tok
        ys_out[h, n] = eos
        n_rows[h] = n + 1
    return ys_in, ys_out, n_rows


def seq_score(logits, targets):
    """sum_l log_softmax(logits[l])[targets[l]] over the len(targets) first rows of logits [>= n, V] (float64)"""
    x = np.asarray(logits, dtype=np.float64)
    s = 0.0
    for l, t in enumerate(targets):
        row = x[l]
        m = row.max()
        s += row[t] - (m + math.log(np.exp(row - m).sum()))
    return s


def total(att, ctc, lm, lam, mu, length, penalty=0.0, lamda=5.0):
    t = (1.0 - lam) * att + lam * ctc + (mu * lm if lm is not None else 0.0)
    if penalty:
        t /= ((lamda + length) / (lamda + 1.0)) ** penalty
    return NEG_INF if t != t else t


def order(totals):
    """rank -> slot: total descending, ties -> lower slot (-inf entries thereby last, in slot order)"""
    return sorted(range(len(totals)), key=lambda i: (-totals[i], i))


def rescore(beam, att_fn, lam, max_len, lm_fn=None, mu=0.0, penalty=0.0, lamda=5.0, nbest=1):
    """beam: per utterance the W slots [(tokens tuple, ctc score)] in CTC order (score -inf: a dead slot).  att_fn(b, h) / lm_fn(b, h):
    the logits [len(h) + 1, V] of the decoder / the LM on [BOS] + h for utterance b.  Returns per utterance a dict: perm (rank -> slot),
    total / att / lm per slot (None where not rescorable), hyps / scores = the nbest best token tuples and totals."""
    out = []
    for b, slots in enumerate(beam):
        tot, atts, lms = [], [], []
        for h, ctc in slots:
            if not (ctc > NEG_INF and len(h) + 1 <= max_len):
                tot.append(NEG_INF), atts.append(None), lms.append(None)
                continue
            tgt = list(h) + [EOS]
            a = seq_score(att_fn(b, h), tgt)
            m = seq_score(lm_fn(b, h), tgt) if lm_fn is not None else None
            atts.append(a), lms.append(m)
            tot.append(total(a, ctc, m, lam, mu, len(h), penalty, lamda))
        perm = order(tot)
        out.append({'perm': perm, 'total': tot, 'att': atts, 'lm': lms, 'hyps': [tuple(slots[i][0]) for i in perm[:nbest]],
                    'scores': [tot[i] for i in perm[:nbest]]})
    return out


def beam_of(tokens, out_len, scores):
    """the search's arrays -> the `beam` argument of rescore"""
    tokens, out_len, scores = np.asarray(tokens), np.asarray(out_len), np.asarray(scores, dtype=np.float64)
    return [[(tuple(int(t) for t in tokens[b, w, :int(out_len[b, w])]), float(scores[b, w])) for w in range(tokens.shape[1])]
            for b in range(tokens.shape[0])]
