"""Plain-Python restatement of phrase biasing (include/otrans_hip.h otr_bias_score_cands / otr_bias_score_seqs;
SpeechToTextRecognizer bias=...).  It does not import opentransformer_amd.bias and builds no trie: whether a string is a node is
asked of the phrase list itself, and psi_minus / psi follow their definitions.  f32 where the contract says f32.  The search is the
n-gram fusion's restatement (tests/ngram_attn_ref.py) with the phrase addend at the candidate stage, behind the n-gram's if any."""
import math

import numpy as np
import torch

from tests.ctc_prefix_score_ref import NEG, _order, extend, start_state
from tests.ngram_attn_ref import _cut_gap, _total
from tests.ngram_attn_ref import addend as ngram_addend

F32 = np.float32
MAX_LEN = 16


class RefBias:
    """phrases: id tuples; weights: one per phrase (duplicates merge with the larger weight, which max() below does by itself)"""

    def __init__(self, phrases, weights, V, eos=1):
        self.phrases = [tuple(int(v) for v in p) for p in phrases]
        self.weights = [F32(w) for w in weights]
        self.V, self.eos = V, eos
        self._memo = {}

    def is_node(self, u):
        return len(u) == 0 or any(p[:len(u)] == u for p in self.phrases)

    def is_end(self, u):
        return len(u) > 0 and u in self.phrases

    def tok(self, u):
        """the largest weight among the phrases that pass through the edge into u"""
        return max(w for p, w in zip(self.phrases, self.weights) if p[:len(u)] == u)

    def psi_minus(self, u):
        above = [m for m in range(1, len(u)) if self.is_end(u[:m])]
        acc = F32(0)
        for d in range((above[-1] if above else 0) + 1, len(u) + 1):      # root to leaf, f32
            acc = F32(acc + self.tok(u[:d]))
        return acc

    def psi(self, u):
        return F32(0) if self.is_end(u) or not u else self.psi_minus(u)

    def state(self, x):
        """the longest suffix of the token string x that is a node (the empty tuple: the root)"""
        x = tuple(int(v) for v in x)
        for j in range(min(len(x), MAX_LEN), 0, -1):
            if self.is_node(x[len(x) - j:]):
                return x[len(x) - j:]
        return ()

    def addend(self, g, c):
        """a(g, c) = psi_minus(state(g c)) - psi(state(g)): one f32 subtraction; EOS leads to the root"""
        g = tuple(int(v) for v in g)[-MAX_LEN:]
        key = (g, int(c))
        if key not in self._memo:
            new = () if c == self.eos else self.state(g + (int(c),))
            self._memo[key] = F32(self.psi_minus(new) - self.psi(self.state(g)))
        return self._memo[key]


def addend(bias, prefix, c):
    return float(bias.addend(prefix, c))


def score_candidates(bias, preds, t, cand_idx, cand_score, eos, flags=None, beam=0):
    """tests/ngram_attn_ref.score_candidates with the phrase addend: rows with flags[r] are copied unchanged (addend 0); a -inf score
    stays -inf; out = cs + a is one f32 addition.  beam > 0: per row the `beam` best totals, descending, ties -> lower token (then the
    lower slot), NaN ranking as -inf; a finished row gets -inf / eos."""
    out, add, ks, ki = [], [], [], []
    for r, (ci, cs) in enumerate(zip(cand_idx, cand_score)):
        fin = bool(flags[r]) if flags is not None else False
        prefix = [int(v) for v in preds[r][1:t]]
        a = [0.0 if fin else addend(bias, prefix, int(c)) for c in ci]
        o = [float(s) if fin else _total(float(s), x) for s, x in zip(cs, a)]
        out.append(o), add.append(a)
        if beam > 0:
            v = [NEG if x != x else x for x in o]
            order = sorted(range(len(ci)), key=lambda i: (-v[i], int(ci[i]), i))[:beam]
            ks.append([NEG if fin else v[i] for i in order])
            ki.append([eos if fin else int(ci[i]) for i in order])
    return out, add, (ks if beam > 0 else None), (ki if beam > 0 else None)


def addends(bias, tokens, eos):
    """the addends of tokens + [EOS], position by position"""
    h = [int(v) for v in tokens]
    return [bias.addend(h[:l], c) for l, c in enumerate(h + [eos])]


def seq_score(bias, tokens, eos):
    """the summed addends of tokens + [EOS], f32, in the order the header states: lane i of 64 adds the positions i, i + 64, .. in
    ascending order from 0, then the lane sums meet in the butterfly v_i += v_(i xor o), o = 32, 16, 8, 4, 2, 1"""
    acc = np.zeros(64, F32)
    for l, a in enumerate(addends(bias, tokens, eos)):
        acc[l % 64] = F32(acc[l % 64] + a)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lanes ^ o]).astype(F32)
    return acc[0]


def banked(bias, tokens):
    """(the psi_minus(v) of every step of the string that landed on an end node v, psi of the final state)"""
    h = [int(v) for v in tokens]
    got = []
    for l in range(1, len(h) + 1):
        s = bias.state(h[:l])
        if bias.is_end(s):
            got.append(bias.psi_minus(s))
    return got, bias.psi(bias.state(h))


def beam_search(att_fn, B, beam, max_len, eos, bias, ngram=None, lm_fn=None, lm_weight=0.0, joint=None, penalty=0.0, lamda=5, nbest=1,
                gaps=None, finished=None):
    """tests/ngram_attn_ref.beam_search with the phrase addend.  bias = dict(ref=RefBias, K=K'); ngram = None or that restatement's
    dict(lm=, alpha=, beta=, K=K') with the same K'.  Plain (joint None): per unfinished row the K' tokens of highest att + lm_weight *
    lm, each plus the n-gram's addend (one f32 addition), then plus the phrase addend (one more), the beam best kept (ties -> lower
    token); joint: both addends enter the K' = joint['K'] pre-beam scores before lambda * (psi(h) - psi(g)) is added.  gaps / finished:
    as there.  Returns (hyps [B][nbest] token lists, scores [B, nbest])."""
    rb = bias['ref']
    R = B * beam
    preds = torch.full((R, 1), eos, dtype=torch.long)
    scores = [0.0 if r % beam == 0 else NEG for r in range(R)]
    flag = [False] * R
    states, lam, K = None, 0.0, bias['K']
    assert ngram is None or ngram['K'] == K
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
            tot = [s[c] for c in cands]
            if ngram is not None:
                tot = [_total(v, ngram_addend(ngram['lm'], prefix, c, ngram['alpha'], ngram['beta'], eos)) for v, c in zip(tot, cands)]
            tot = [_total(v, addend(rb, prefix, c)) for v, c in zip(tot, cands)]
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
