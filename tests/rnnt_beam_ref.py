"""The transducer's beam search (include/otrans_hip.h, otr_rnnt_beam_select) restated in plain torch and Python, dtype-generic like
tests/rnnt_ref.py: run it in float64 for a reference, in float32 for the rounding floor of that very computation.  blank = 0.

  beam_frame      one frame of one utterance: a dict of candidates keyed by the token tuple, the merge, the tie rule
  rnnt_beam_ref   the search of ONE utterance over rnnt_greedy_ref's callbacks (rnnt_ref.TransducerRef.predict / joint_logits)
  beam_step_ref   one frame with the select kernel's inputs and outputs (W slots, dead ones included)
  enumerate_ref   the log-sum over ALL alignments of the one-symbol-per-frame lattice, per token sequence (tiny cases only)
"""
import itertools

import torch

BLANK = 0
INF = float('inf')


def beam_frame(hyps, lps, t, W, max_len):
    """hyps: the live hypotheses in slot order, [(slot, tokens tuple, frames tuple, score 0-d tensor)], distinct token tuples; lps: their
    log-softmax rows.  -> (new beam best first [(tokens, frames, score, parent slot, step token)], gap between candidate W and W + 1
    (inf if there is none), merges).  A candidate's sort key is the tie rule: score down, a stay before an extension, the lower
    parent slot, the lower token."""
    cands, merges = {}, 0
    for (slot, y, fr, s), lp in zip(hyps, lps):                                    # the stays first: a merge joins an extension to one
        cands[y] = dict(score=s + lp[BLANK], kind=0, parent=slot, tok=BLANK, tokens=y, frames=fr)
    for (slot, y, fr, s), lp in zip(hyps, lps):
        if len(y) >= max_len:
            continue
        for k in range(lp.shape[0]):
            if k == BLANK:
                continue
            key, e = y + (k,), s + lp[k]
            if key in cands:                                                       # keeps the stay's frames, slot and predictor state
                assert cands[key]['kind'] == 0
                cands[key]['score'] = torch.logaddexp(cands[key]['score'], e)
                merges += 1
            else:
                cands[key] = dict(score=e, kind=1, parent=slot, tok=k, tokens=key, frames=fr + (t,))
    order = sorted(cands.values(), key=lambda c: (-float(c['score']), c['kind'], c['parent'], c['tok']))
    order = [c for c in order if float(c['score']) > -INF]
    gap = float(order[W - 1]['score'] - order[W]['score']) if len(order) > W else INF
    return [(c['tokens'], c['frames'], c['score'], c['parent'], c['tok']) for c in order[:W]], gap, merges


@torch.no_grad()
def rnnt_beam_ref(pe_b, Tb, predict, joint_logits, W, max_len, bos=1):
    """The beam search of ONE utterance.  pe_b [T, J]; predict(token, state) -> (pg [J], state) (state None: zero); joint_logits(pe_t,
    pg) -> logits [V].  Returns (hypotheses best first [(tokens list, frames list, score float)], min_gap: the smallest difference
    between the W-th and the (W + 1)-th candidate over all frames and between neighbours of the final beam, merges)."""
    pg, state = predict(bos, None)
    beam = [((), (), pe_b.new_zeros(()), pg, state)]
    min_gap, merges = INF, 0
    for t in range(Tb):
        hyps = [(i, y, fr, s) for i, (y, fr, s, _, _) in enumerate(beam)]
        lps = [torch.log_softmax(joint_logits(pe_b[t], h[3]), dim=-1) for h in beam]
        new, gap, m = beam_frame(hyps, lps, t, W, max_len)
        min_gap, merges = min(min_gap, gap), merges + m
        nxt = []
        for y, fr, s, parent, tok in new:
            pg, state = beam[parent][3], beam[parent][4]
            if tok != BLANK:
                pg, state = predict(tok, state)
            nxt.append((y, fr, s, pg, state))
        beam = nxt
    for a, b in zip(beam, beam[1:]):
        min_gap = min(min_gap, float(a[2] - b[2]))
    return [(list(y), list(fr), float(s)) for y, fr, s, _, _ in beam], min_gap, merges


@torch.no_grad()
def beam_step_ref(logits, t, score, n, tokens, frames, max_len):
    """One frame with the select kernel's inputs and outputs.  logits [W, >= V] (only [:, :V] is passed in), score [W] (-inf: dead), n
    [W], tokens / frames [W, max_len].  -> dict(parent, step_tok, emit, n: int lists [W]; score: tensor [W]; tokens, frames: lists of
    lists (the live part); gap)."""
    W = logits.shape[0]
    hyps = [(i, tuple(tokens[i, :int(n[i])].tolist()), tuple(frames[i, :int(n[i])].tolist()), score[i]) for i in range(W) if float(score[i]) > -INF]
    lps = [torch.log_softmax(logits[i], dim=-1) for i, _, _, _ in hyps]
    new, gap, merges = beam_frame(hyps, lps, t, W, max_len)
    out = dict(parent=list(range(W)), step_tok=[BLANK] * W, emit=[0] * W, n=[0] * W, score=logits.new_full((W,), -INF),
               tokens=[[] for _ in range(W)], frames=[[] for _ in range(W)], gap=gap, merges=merges)
    for r, (y, fr, s, parent, tok) in enumerate(new):
        out['parent'][r], out['step_tok'][r], out['emit'][r], out['n'][r] = parent, tok, int(tok != BLANK), len(y)
        out['score'][r], out['tokens'][r], out['frames'][r] = s, list(y), list(fr)
    return out


@torch.no_grad()
def enumerate_ref(pe_b, Tb, predict, joint_logits, V, max_len=None, bos=1):
    """{token tuple: log of the summed probability of ALL its alignments} over the lattice in which every frame emits blank or exactly
    one token: V ** Tb paths (those of more than max_len tokens left out), each scored on its own (nothing is shared with the search
    but the callbacks)"""
    total = {}
    for path in itertools.product(range(V), repeat=Tb):
        if max_len is not None and sum(k != BLANK for k in path) > max_len:
            continue
        pg, state = predict(bos, None)
        lp_sum, y = pe_b.new_zeros(()), ()
        for t, k in enumerate(path):
            lp_sum = lp_sum + torch.log_softmax(joint_logits(pe_b[t], pg), dim=-1)[k]
            if k != BLANK:
                y = y + (k,)
                pg, state = predict(k, state)
        total.setdefault(y, []).append(lp_sum)
    return {y: float(torch.logsumexp(torch.stack(v), dim=0)) for y, v in total.items()}


def table_model(V=3, J=4, T=3, seed=0, dtype=torch.float64, scale=1.0):
    """a table-driven transducer for the enumeration: the predictor's state is the id of the history (empty 0, id' = (V - 1) * id + k),
    its projection a row of a random table; -> (pe [T, J], table [ids, J], weight [V, J], bias [V])"""
    g = torch.Generator().manual_seed(seed)
    ids = sum((V - 1) ** i for i in range(T + 2))
    pe = torch.randn((T, J), generator=g, dtype=torch.float64)
    table = torch.randn((ids, J), generator=g, dtype=torch.float64)
    weight = torch.randn((V, J), generator=g, dtype=torch.float64) * scale
    bias = torch.randn((V,), generator=g, dtype=torch.float64)
    return pe.to(dtype), table.to(dtype), weight.to(dtype), bias.to(dtype)


def table_callbacks(table, weight, bias):
    """(predict, joint_logits) of table_model for rnnt_beam_ref / enumerate_ref"""
    V = weight.shape[0]

    def predict(token, state):
        hid = 0 if state is None else (V - 1) * state + token
        return table[hid], hid

    def joint_logits(pe_t, pg):
        return torch.nn.functional.linear(torch.tanh(pe_t + pg), weight, bias)
    return predict, joint_logits
