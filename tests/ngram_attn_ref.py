"""Plain-Python restatement of the n-gram LM fusion of the attention, joint and two-pass decoders (include/otrans_hip.h
otr_ngram_score_cands / otr_ngram_score_seqs; SpeechToTextRecognizer ngram_lm=...).  Built on the joint search's restatement
(tests/ctc_prefix_score_ref.py) and the backoff rule's (tests/ngram_ref.py RefLM), neither of which it changes.

The context of a hypothesis whose prefix row is [BOS, y_1 .. y_{t-1}] is <s> y_1 .. y_{t-1} cut to its last order-1 ids: column 0 is
<s> by position (BOS == EOS, so its value says nothing).  The addend of candidate c is alpha * ln P(c | context) + (c == eos ? 0 :
beta), rounded to f32 after the product and after the sum as the device rounds it; ln P itself is RefLM's float64."""
import math

import numpy as np
import torch

from tests.ctc_prefix_score_ref import NEG, _order, extend, start_state

F32 = np.float32


def addend(lm, prefix, c, alpha, beta, eos):
    """a(g, c) for the hypothesis whose tokens behind BOS are `prefix`"""
    a = F32(alpha) * F32(lm.cond(lm.context(prefix), c))
    return float(a if c == eos else F32(a + F32(beta)))


def _total(cs, a):
    if cs != cs:
        return cs
    return NEG if cs == NEG else float(F32(F32(cs) + F32(a)))


def score_candidates(lm, preds, t, cand_idx, cand_score, alpha, beta, eos, flags=None, beam=0):
    """The candidate scorer.  preds [R][>= t] prefix rows (column 0 = BOS), cand_idx / cand_score [R][K].  Returns (cand_out, cand_add,
    k_score, k_idx): rows with flags[r] are copied unchanged (addend 0); a -inf score stays -inf.  beam > 0: per row the `beam` best
    totals, descending, ties -> lower token (then the lower slot), NaN ranking as -inf; a finished row gets -inf / eos.  beam = 0:
    k_score = k_idx = None."""
    out, add, ks, ki = [], [], [], []
    for r, (ci, cs) in enumerate(zip(cand_idx, cand_score)):
        fin = bool(flags[r]) if flags is not None else False
        prefix = [int(v) for v in preds[r][1:t]]
        a = [0.0 if fin else addend(lm, prefix, int(c), alpha, beta, eos) for c in ci]
        o = [float(s) if fin else _total(float(s), x) for s, x in zip(cs, a)]
        out.append(o), add.append(a)
        if beam > 0:
            v = [NEG if x != x else x for x in o]
            order = sorted(range(len(ci)), key=lambda i: (-v[i], int(ci[i]), i))[:beam]
            ks.append([NEG if fin else v[i] for i in order])
            ki.append([eos if fin else int(ci[i]) for i in order])
    return out, add, (ks if beam > 0 else None), (ki if beam > 0 else None)


def seq_score(lm, tokens, alpha, beta, eos, with_logp=False):
    """ng(h) = alpha * (sum_l ln P(h_l | context(h_{<l})) + ln P(</s> | context(h))) + beta * |h|, float64"""
    h = [int(v) for v in tokens]
    logp = sum(lm.cond(lm.context(h[:j]), c) for j, c in enumerate(h + [eos]))
    s = alpha * logp + beta * len(h)
    return (s, logp) if with_logp else s


def _cut_gap(sorted_vals, keep):
    """distance between the last kept and the first dropped of a descending list (inf where nothing finite is dropped)"""
    if keep >= len(sorted_vals) or sorted_vals[keep] == NEG:
        return math.inf
    return sorted_vals[keep - 1] - sorted_vals[keep]


def beam_search(att_fn, B, beam, max_len, eos, ngram, lm_fn=None, lm_weight=0.0, joint=None, penalty=0.0, lamda=5, nbest=1,
                gaps=None, finished=None):
    """ctc_prefix_score_ref.beam_search with the n-gram's addend at the candidate stage.  ngram = dict(lm=RefLM, alpha=, beta=, K=K'):
    plain (joint None): per unfinished row the K' tokens of highest att + lm_weight * lm, each plus its addend, the beam best kept
    (ties -> lower token); joint: the addend enters the K' = joint['K'] pre-beam scores before lambda * (psi(h) - psi(g)) is added.
    Everything is formed in f32 where the device forms it in f32.  gaps (a list) receives, per step, the smallest distance between
    the last kept and the first dropped entry of the pre-beam cut, the per-row cut and the beam^2 prune, and at the end that between
    neighbours of the returned n-best; finished (a list) receives
    every (utterance, token list without EOS, score) the moment a hypothesis ends in EOS.
    Returns (hyps [B][nbest] token lists, scores [B, nbest])."""
    lm_ng, alpha, beta = ngram['lm'], ngram['alpha'], ngram['beta']
    R = B * beam
    preds = torch.full((R, 1), eos, dtype=torch.long)
    scores = [0.0 if r % beam == 0 else NEG for r in range(R)]
    flag = [False] * R
    states, lam, K = None, 0.0, ngram['K']
    if joint is not None:
        lam, K = float(joint['ctc_weight']), joint['K']
        Tbs = [max(1, min(int(joint['lengths'][b]), len(joint['x'][b]))) for b in range(B)]
        states = [start_state(joint['x'][r // beam], Tbs[r // beam], joint['blank']) for r in range(R)]
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    for _ in range(max_len):
        att = att_fn(preds).float()
        lm = lm_fn(preds).float() if lm_fn is not None else None
        k_scores, k_preds, k_states = [], [], []
        step_gap = math.inf
        for r in range(R):
            if flag[r]:
                k_scores.append([0.0] + [NEG] * (beam - 1))
                k_preds.append([eos] * beam)
                k_states.append([None] * beam)
                continue
            s = att[r] * t32(1.0 - lam) if joint is not None else att[r]
            if lm is not None:
                s = s + t32(lm_weight) * lm[r]
            s = s.tolist()
            full = _order(s)
            cands = full[:K]
            live = scores[r] > NEG
            if live:
                step_gap = min(step_gap, _cut_gap([s[i] for i in full], K))
            prefix = preds[r, 1:].tolist()
            tot = [_total(s[c], addend(lm_ng, prefix, c, alpha, beta, eos)) for c in cands]
            sts = [None] * len(cands)
            if joint is not None:
                b = r // beam
                psi_g = states[r][2] if states[r] is not None else NEG
                js = []
                for i, c in enumerate(cands):
                    psi, sts[i] = extend(states[r], joint['x'][b], Tbs[b], c, joint['blank'], eos)
                    if lam == 0.0:
                        j = tot[i]
                    elif psi == NEG or psi_g == NEG:
                        j = NEG
                    else:
                        j = float(t32(tot[i]) + t32(lam) * t32(psi - psi_g))
                    js.append(j)
                tot = js
            order = sorted(range(len(cands)), key=lambda i: (-tot[i], cands[i]))
            if live:
                step_gap = min(step_gap, _cut_gap([tot[i] for i in order], beam))
            order = order[:beam]
            pad = beam - len(order)                           # beam > K' (the brute-force check only): entries that cannot win
            k_scores.append([tot[i] for i in order] + [NEG] * pad)
            k_preds.append([cands[i] for i in order] + [eos] * pad)
            k_states.append([sts[i] for i in order] + [None] * pad)
        new_preds, new_scores, new_flag, new_states = [], [], [], []
        for b in range(B):
            cand = []
            for h in range(beam):
                r = b * beam + h
                for br in range(beam):
                    cand.append(float(t32(scores[r]) + t32(k_scores[r][br])))
            ranked = _order(cand)
            step_gap = min(step_gap, _cut_gap([cand[i] for i in ranked], beam))
            for w in ranked[:beam]:
                src, br = b * beam + w // beam, w % beam
                tok = eos if flag[src] else k_preds[src][br]
                new_preds.append(torch.cat([preds[src], torch.tensor([tok])]))
                new_scores.append(cand[w])
                new_flag.append(tok == eos)
                if finished is not None and tok == eos and not flag[src] and cand[w] > NEG:
                    finished.append((b, preds[src, 1:].tolist(), cand[w]))
                if states is not None:
                    new_states.append(states[src] if flag[src] else k_states[src][br])
        preds, scores, flag = torch.stack(new_preds), new_scores, new_flag
        states = new_states if states is not None else None
        if gaps is not None:
            gaps.append(step_gap)
        if all(flag):
            break
    sc = torch.tensor(scores, dtype=torch.float32).view(B, beam)
    pv = preds.view(B, beam, -1)
    if penalty:
        lengths = (pv != eos).float().sum(-1)
        sc = sc / torch.pow((lamda + lengths) / (lamda + 1), penalty)
    ss, idx = torch.sort(sc, dim=-1, descending=True, stable=True)
    if gaps is not None:                                      # the n-best selection is a cut too
        gaps.append(min(_cut_gap(ss[b, :n + 2].tolist(), n + 1) for b in range(B) for n in range(min(beam, nbest))))
    pv = torch.gather(pv, 1, idx.unsqueeze(-1).expand_as(pv))[:, :min(beam, nbest), 1:]
    hyps = []
    for b in range(B):
        row = []
        for n in range(pv.size(1)):
            out = []
            for t in pv[b, n].tolist():
                if t == eos:
                    break
                out.append(t)
            row.append(out)
        hyps.append(row)
    return hyps, ss[:, :min(beam, nbest)]
