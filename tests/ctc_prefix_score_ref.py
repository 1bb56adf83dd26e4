"""Plain-Python restatement of the joint CTC/attention beam search (include/otrans_hip.h otr_joint_prebeam / otr_ctc_prefix_score,
recognize.SpeechToTextRecognizer joint_ctc=True; Watanabe et al. 2017, Algorithm 2).  Log space throughout, float64; "+" of
probabilities is log-add-exp.  x[t][c] is the CTC log-prob of token c at frame t, Tb the utterance's frames.

A prefix state is (r^n [Tb], r^b [Tb], psi, last token or None for the start prefix)."""
import math

import torch

NEG = -math.inf


def lae(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log1p(math.exp(min(a, b) - m))


def start_state(x, Tb, blank):
    """the start prefix (BOS only): r^n = -inf, r^b_t = sum_{tau <= t} x_tau(blank), psi = 0, no last token"""
    rb, a = [], 0.0
    for t in range(Tb):
        a += x[t][blank]
        rb.append(a)
    return [NEG] * Tb, rb, 0.0, None


def extend(state, x, Tb, c, blank, eos):
    """(psi(h), state of h) for h = g.c; the state is None for blank and EOS, whose prefix probability is 0 (-inf) and so is that
    of every extension (only a search at lambda = 0 ever keeps such a hypothesis)"""
    if state is None:
        return NEG, None
    rn_g, rb_g, _, last = state
    if c == blank:
        return NEG, None
    if c == eos:
        return lae(rn_g[Tb - 1], rb_g[Tb - 1]), None
    phi = [rb_g[t] if c == last else lae(rn_g[t], rb_g[t]) for t in range(Tb)]
    rn, rb = [NEG] * Tb, [NEG] * Tb
    rn[0] = x[0][c] if last is None else NEG
    psi = rn[0]
    for t in range(1, Tb):
        rn[t] = lae(rn[t - 1], phi[t - 1]) + x[t][c]
        rb[t] = lae(rb[t - 1], rn[t - 1]) + x[t][blank]
        psi = lae(psi, phi[t - 1] + x[t][c])
    return psi, (rn, rb, psi, c)


def prefix_state(x, Tb, prefix, blank, eos):
    """state of the prefix BOS + `prefix` (tokens that are neither blank nor EOS)"""
    st = start_state(x, Tb, blank)
    for c in prefix:
        _, st = extend(st, x, Tb, c, blank, eos)
    return st


def prefix_scores(x, Tb, prefix, cands, blank, eos):
    st = prefix_state(x, Tb, prefix, blank, eos)
    return [extend(st, x, Tb, c, blank, eos)[0] for c in cands]


def _order(scores):
    """indices in descending score order, ties -> lower index"""
    return sorted(range(len(scores)), key=lambda i: (-scores[i], i))


def beam_search(att_fn, B, beam, max_len, eos, lm_fn=None, lm_weight=0.0, joint=None, penalty=0.0, lamda=5, nbest=1):
    """The batch beam search of recognize.py / oracle.beam_search (finished-beam masking, beam^2 -> beam prune), optionally joint.
    att_fn(preds [R, t] long) -> att log-probs [R, V]; lm_fn likewise (or None).  joint = None (plain: top-beam of att + lm_weight * lm)
    or dict(x=[B][T][V] CTC log-probs, lengths=[B], ctc_weight=lambda, K=K', blank=blank).  The pre-beam and joint scores are formed in
    f32 as the device does: (1 - lambda) * att + lm_weight * lm, then + lambda * (psi(h) - psi(g)).
    Returns (hyps [B][nbest] token lists, scores [B, nbest])."""
    R = B * beam
    preds = torch.full((R, 1), eos, dtype=torch.long)
    scores = [0.0 if r % beam == 0 else NEG for r in range(R)]
    flag = [False] * R
    states = None
    if joint is not None:
        lam = float(joint['ctc_weight'])
        Tbs = [max(1, min(int(joint['lengths'][b]), len(joint['x'][b]))) for b in range(B)]
        states = [start_state(joint['x'][r // beam], Tbs[r // beam], joint['blank']) for r in range(R)]
    for _ in range(max_len):
        att = att_fn(preds).float()
        lm = lm_fn(preds).float() if lm_fn is not None else None
        k_scores, k_preds, k_states = [], [], []
        for r in range(R):
            if flag[r]:
                k_scores.append([0.0] + [NEG] * (beam - 1))
                k_preds.append([eos] * beam)
                k_states.append([None] * beam)
                continue
            if joint is None:
                s = att[r] + lm_weight * lm[r] if lm is not None else att[r]
                s = s.tolist()
                top = _order(s)[:beam]
                k_scores.append([s[i] for i in top])
                k_preds.append(top)
                k_states.append([None] * beam)
                continue
            s = att[r] * torch.tensor(1.0 - lam, dtype=torch.float32)
            if lm is not None:
                s = s + torch.tensor(lm_weight, dtype=torch.float32) * lm[r]
            s = s.tolist()
            cands = _order(s)[:joint['K']]
            b = r // beam
            psi_g = states[r][2] if states[r] is not None else NEG
            js, sts = [], []
            for c in cands:
                psi, st = extend(states[r], joint['x'][b], Tbs[b], c, joint['blank'], eos)
                if lam == 0.0:
                    j = s[c]
                elif psi == NEG or psi_g == NEG:
                    j = NEG
                else:
                    j = float(torch.tensor(s[c], dtype=torch.float32) + torch.tensor(lam, dtype=torch.float32)
                              * torch.tensor(psi - psi_g, dtype=torch.float32))
                js.append(j)
                sts.append(st)
            order = sorted(range(len(cands)), key=lambda i: (-js[i], cands[i]))[:beam]
            k_scores.append([js[i] for i in order])
            k_preds.append([cands[i] for i in order])
            k_states.append([sts[i] for i in order])
        new_preds, new_scores, new_flag, new_states = [], [], [], []
        for b in range(B):
            cand = []
            for h in range(beam):
                r = b * beam + h
                for br in range(beam):
                    cand.append(float(torch.tensor(scores[r], dtype=torch.float32) + torch.tensor(k_scores[r][br], dtype=torch.float32)))
            for w in _order(cand)[:beam]:
                src, br = b * beam + w // beam, w % beam
                tok = eos if flag[src] else k_preds[src][br]
                new_preds.append(torch.cat([preds[src], torch.tensor([tok])]))
                new_scores.append(cand[w])
                new_flag.append(tok == eos)
                if states is not None:
                    new_states.append(states[src] if flag[src] else k_states[src][br])
        preds, scores, flag = torch.stack(new_preds), new_scores, new_flag
        states = new_states if states is not None else None
        if all(flag):
            break
    sc = torch.tensor(scores, dtype=torch.float32).view(B, beam)
    pv = preds.view(B, beam, -1)
    if penalty:
        lengths = (pv != eos).float().sum(-1)
        sc = sc / torch.pow((lamda + lengths) / (lamda + 1), penalty)
    ss, idx = torch.sort(sc, dim=-1, descending=True, stable=True)
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
