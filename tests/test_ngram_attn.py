"""CPU (-m "not gpu"): the n-gram LM fusion of the attention, joint and two-pass decoders (SpeechToTextRecognizer ngram_lm=...).  The
restatement (tests/ngram_attn_ref.py) is checked against brute force -- with nothing pruned every finished hypothesis scores
(1 - lambda) ln P_att + lambda ln P_ctc + alpha ln P_ng(h </s>) + beta |h| -- its candidate scorer against hand-made rows, its
sentence score against the sum of RefLM lookups and the host walk of the device table; the recognizer and the library's entry points
refuse what is outside the documented limits before they launch."""
import ctypes as C
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from opentransformer_amd.ngram import NGramLM
from tests import ngram_attn_ref as ref
from tests.ngram_cases import lm_pair

BLANK, EOS = 0, 1
NEG = -math.inf


def rand_lp(rng, T, V, peak=2.0):
    lp = rng.normal(size=(T, V)) * peak
    return (lp - np.log(np.exp(lp).sum(-1, keepdims=True))).tolist()


def collapse(path):
    out, last = [], None
    for c in path:
        if c != last and c != BLANK:
            out.append(c)
        last = c
    return tuple(out)


def att_table(V, max_len, seed):
    """a fixed table {prefix tuple: log-probs [V]} over every prefix of up to max_len tokens, and the att_fn that reads it"""
    rng = np.random.default_rng(seed)
    table = {}
    for n in range(max_len + 1):
        for g in itertools.product(range(V), repeat=n):
            x = rng.normal(size=V) * 1.5
            table[g] = torch.tensor(x - np.log(np.exp(x).sum()), dtype=torch.float32)
    return table, lambda preds: torch.stack([table[tuple(row[1:])] for row in preds.tolist()])


@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_unpruned_search_scores_the_identity(order, mode):
    """V = 4, max_len = 3, K' = V, beam 64 >= the 4^3 strings: nothing is pruned, so every hypothesis that ended in EOS carries the
    sum of the contract, each term computed here by brute force (the attention table, every CTC alignment, RefLM.score).  The search
    adds in f32: the bound is 16 roundings of 2^-24 relative to the sum of the terms' magnitudes."""
    V, max_len, beam, T = 4, 3, 64, 4
    alpha, beta, lam = 0.7, 0.4, (0.3 if mode == 'joint' else 0.0)
    _, lm = lm_pair(order, V, order, (6, 8)[:order - 1])
    table, att_fn = att_table(V, max_len, 3 + order)
    rng = np.random.default_rng(17)
    x = rand_lp(rng, T, V)
    joint = dict(x=[x], lengths=[T], ctc_weight=lam, K=V, blank=BLANK) if mode == 'joint' else None
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        key = collapse(path)
        mass[key] = mass.get(key, 0.0) + math.exp(sum(x[t][c] for t, c in enumerate(path)))
    done = []
    ref.beam_search(att_fn, 1, beam, max_len, EOS, dict(lm=lm, alpha=alpha, beta=beta, K=V), joint=joint, nbest=beam, finished=done)
    seen = set()
    for _, h, score in done:
        h = tuple(h)
        assert h not in seen and EOS not in h
        seen.add(h)
        terms = [(1.0 - lam) * float(table[h[:l]][c]) for l, c in enumerate(h + (EOS,))]
        if mode == 'joint':
            assert BLANK not in h and mass.get(h, 0.0) > 0.0      # a string CTC cannot emit never ends with a finite score
            terms.append(lam * math.log(mass[h]))
        terms += [alpha * lm.score(list(h) + [EOS]), beta * len(h)]
        assert abs(score - sum(terms)) <= 16 * 2.0 ** -24 * sum(abs(v) for v in terms) + 1e-9, (h, score, sum(terms))
    if mode == 'plain':                                           # every string of < max_len tokens over the 3 non-EOS units ended
        assert seen == {g for n in range(max_len) for g in itertools.product((0, 2, 3), repeat=n)}
    else:                                                         # ... over the units CTC can emit, where T frames hold them
        want = {g for n in range(max_len) for g in itertools.product((2, 3), repeat=n) if mass.get(g, 0.0) > 0.0}
        assert seen == want and len(seen) >= 6


def test_alpha_beta_zero_is_the_search_without_an_ngram():
    """at alpha = beta = 0 and K' = V the restatement is the joint search's own restatement, plain and joint"""
    from tests import ctc_prefix_score_ref as base
    V, B, beam = 6, 2, 3
    _, lm = lm_pair(2, V, 2, (8,))
    _, att_fn = att_table(V, 4, 9)
    rng = np.random.default_rng(2)
    for joint in (None, dict(x=[rand_lp(rng, 7, V) for _ in range(B)], lengths=[7, 3], ctc_weight=0.4, K=V, blank=BLANK)):
        h0, s0 = base.beam_search(att_fn, B, beam, 4, EOS, joint=joint, nbest=beam)
        h1, s1 = ref.beam_search(att_fn, B, beam, 4, EOS, dict(lm=lm, alpha=0.0, beta=0.0, K=V), joint=joint, nbest=beam)
        assert h0 == h1 and torch.equal(s0, s1)
        h2, _ = ref.beam_search(att_fn, B, beam, 4, EOS, dict(lm=lm, alpha=2.0, beta=0.0, K=V), joint=joint, nbest=beam)
        assert h2 != h0                                           # and the n-gram is consulted otherwise


def test_candidate_scorer_rules():
    """addend, EOS without beta, column 0 as <s> by position, ties to the lower token, a finished row, -inf staying -inf"""
    V = 6
    _, lm = lm_pair(4, V, 3, (10, 12))
    alpha, beta = 0.5, 1.25
    preds = [[EOS, 2, 3], [EOS, 2, 3], [EOS, EOS, 5]]
    cand_idx = [[3, EOS, 2, 4], [3, EOS, 2, 4], [4, 2, 5, EOS]]
    cand_score = [[-1.0, -2.0, NEG, -0.5], [-1.0, -2.0, NEG, -0.5], [-1.0, -1.0, -1.0, -1.0]]
    out, add, ks, ki = ref.score_candidates(lm, preds, 3, cand_idx, cand_score, alpha, beta, EOS, flags=[0, 1, 0], beam=3)
    for k, c in enumerate(cand_idx[0]):
        want = alpha * lm.cond((V, 2, 3)[-2:], c) + (0.0 if c == EOS else beta)
        assert abs(add[0][k] - want) <= 1e-6 * abs(want) + 1e-6
    assert out[0][2] == NEG and all(o == o for row in out for o in row)
    assert out[1] == cand_score[1] and add[1] == [0.0] * 4 and ks[1] == [NEG] * 3 and ki[1] == [EOS] * 3
    assert ks[0] == sorted((o for o in out[0]), reverse=True)[:3] and NEG not in ks[0]
    # row 2: the prefix [BOS, EOS-valued token, 5] -- only column 0 is <s>; column 1 holds the unit EOS = 1 as an ordinary id
    assert abs(add[2][1] - (alpha * lm.cond((1, 5), 2) + beta)) <= 1e-5
    # t = 1: <s> alone, whatever column 0 holds
    _, add1, _, _ = ref.score_candidates(lm, [[EOS]], 1, [[2]], [[0.0]], alpha, beta, EOS)
    assert abs(add1[0][0] - (alpha * lm.cond((V,), 2) + beta)) <= 1e-5
    # equal totals: the lower token first, whatever the slot order
    flat = NGramFlat()
    _, _, ks, ki = ref.score_candidates(flat, [[EOS]], 1, [[5, 3, 4]], [[-1.0, -1.0, -2.0]], 1.0, 0.0, EOS, beam=2)
    assert ki[0] == [3, 5] and ks[0][0] == ks[0][1]


class NGramFlat:
    """an 'LM' that gives every token the same log-prob: equal candidate scores stay equal"""
    def context(self, prefix):
        return ()

    def cond(self, ctx, c):
        return -1.5


@pytest.mark.parametrize('order', [1, 2, 3, 5])
def test_sentence_score_is_the_sum_of_lookups(order):
    """seq_score = alpha * (the RefLM lookups of every token and of </s>) + beta * len, for the empty hypothesis, one shorter than
    N-1, and longer ones; the same sum from the host walk of the table the device probes, to f32 rounding"""
    V = 50
    dev_lm, lm = lm_pair(order, V, order, (300, 400, 300, 200)[:order - 1])
    rng = np.random.default_rng(order)
    alpha, beta = 0.3, 0.8
    for n in (0, 1, max(order - 2, 0), order - 1 if order > 1 else 2, 12):
        h = [int(v) for v in rng.integers(1, V, size=n)]
        conds = [lm.cond(lm.context(h[:j]), c) for j, c in enumerate(h + [EOS])]
        s, logp = ref.seq_score(lm, h, alpha, beta, EOS, with_logp=True)
        assert abs(logp - sum(conds)) < 1e-9 and abs(logp - lm.score(h + [EOS])) < 1e-9
        assert abs(s - (alpha * sum(conds) + beta * n)) < 1e-9
        host = dev_lm.lookup_host([dev_lm.context(h[:j]) for j in range(n + 1)], h + [EOS])
        assert abs(float(host.astype(np.float64).sum()) - logp) <= 1e-6 * sum(abs(c) for c in conds) + 1e-6 * (n + 1)
    assert ref.seq_score(lm, [], alpha, beta, EOS) == alpha * lm.cond(lm.context([]), EOS)


def test_ngramlm_score_is_the_public_sentence_scorer():
    """NGramLM.score exists, takes (tokens, lengths, alpha, beta) and, like every op here, refuses CPU tensors instead of falling back"""
    lm, _ = lm_pair(2, 50, 2, (300,))
    with pytest.raises(_lib.OtransHipError, match='CUDA/HIP'):
        lm.score(torch.zeros((2, 3), dtype=torch.int64), torch.tensor([3, 1]), alpha=0.5, beta=0.1)


def _model(ctc_weight, V=12):
    dec = SimpleNamespace(output_layer=SimpleNamespace(weight=torch.zeros(V, 4)))
    m = SimpleNamespace(decoder=dec, encoder=SimpleNamespace(), eval=lambda: m)
    if ctc_weight > 0:
        m.assistor = SimpleNamespace(blank=0)
    return m


def test_recognizer_refuses_what_the_fusion_cannot_do():
    from opentransformer_amd.recognize import CTCRecognizer, SpeechToTextRecognizer, build_recognizer
    lm12, _ = lm_pair(2, 12, 2, (20,))
    lm100, _ = lm_pair(2, 100, 2, (300,))
    rec = SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_lm=lm12)
    assert rec.ngram_beam == 6 and (rec.alpha, rec.beta) == (0.1, 0.0)          # min(V, int(1.5 * beam)); CTCRecognizer's defaults
    assert SpeechToTextRecognizer(_model(0.0, V=100), beam_width=10, ngram_lm=lm100).ngram_beam == 15
    none = SpeechToTextRecognizer(_model(0.0), beam_width=4)
    assert none.ngram_lm is None and none.ngram_beam is None
    with pytest.raises(NotImplementedError) as e1:
        SpeechToTextRecognizer(_model(0.0), ngram_lm='lm.arpa')
    with pytest.raises(NotImplementedError) as e2:
        CTCRecognizer(_model(0.3), mode='beam', ngram_lm='lm.arpa')
    assert str(e1.value).split(':', 1)[1] == str(e2.value).split(':', 1)[1]       # the same refusal text
    with pytest.raises(ValueError, match='units'):
        SpeechToTextRecognizer(_model(0.0, V=100), ngram_lm=lm12)
    with pytest.raises(ValueError, match='beam_width'):
        SpeechToTextRecognizer(_model(0.0, V=100), beam_width=17, ngram_lm=lm100)
    for bad in (3, 33):
        with pytest.raises(ValueError, match='ngram_beam'):
            SpeechToTextRecognizer(_model(0.0, V=100), beam_width=4, ngram_beam=bad, ngram_lm=lm100)
    with pytest.raises(ValueError, match='ngram_beam'):
        SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_beam=13, ngram_lm=lm12)       # above V
    big = NGramLM.__new__(NGramLM)                                # the constructor refuses 8193 units itself: the recognizer's own check
    big.vocab_size = 8193
    with pytest.raises(ValueError, match='8192'):
        SpeechToTextRecognizer(_model(0.0, V=8193), ngram_lm=big)
    # the joint and the two-pass modes take the n-gram with their own limits
    assert SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, joint_ctc=True, ngram_lm=lm12).ctc_beam == 6
    assert SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, rescore=True, ngram_lm=lm12).ngram_lm is lm12
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1,
                           ngram_lm=lm12, alpha=0.5, beta=1.0, ngram_beam=8)
    rec = build_recognizer('speech2text', _model(0.3), None, args, None)
    assert rec.ngram_lm is lm12 and (rec.alpha, rec.beta, rec.ngram_beam) == (0.5, 1.0, 8)
    del args.ngram_lm, args.alpha, args.beta, args.ngram_beam
    assert build_recognizer('speech2text', _model(0.3), None, args, None).ngram_lm is None


def test_build_recognizer_loads_an_arpa_path(tmp_path):
    from opentransformer_amd.recognize import build_recognizer
    from tests.ngram_ref import make_lm
    text, _, idx2unit = make_lm(1, 12, 2, [20])
    path = tmp_path / 'lm.arpa'
    path.write_text(text)
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.0, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1, ngram_lm=str(path))
    rec = build_recognizer('speech2text', _model(0.0), None, args, idx2unit)
    assert isinstance(rec.ngram_lm, NGramLM) and rec.ngram_lm.vocab_size == 12 and rec.ngram_lm.order == 2


def test_entry_points_refuse_bad_arguments():
    """checked on the host before any launch (no GPU needed)"""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(C.addressof(buf) + (-C.addressof(buf)) % 32, C.c_void_p)        # 32-byte aligned, as a table must be

    def cands(cap=4, probe=1, order=3, V=100, ldp=10, t=1, pos=None, K=8, eos=1, beam=0, ks=p, alpha=0.5):
        return lib.otr_ngram_score_cands(p, cap, probe, order, V, p, ldp, t, pos, None, p, p, 4, K, alpha, 0.0, -1000.0, eos, p, None,
                                         beam, ks, ks, None)
    assert cands(K=33) != 0 and cands(K=0) != 0
    assert b'ngram_score_cands' in lib.otr_last_error_string()
    assert cands(beam=17, K=20) != 0 and cands(beam=9, K=8) != 0 and cands(beam=4, ks=None) != 0
    assert cands(t=0) != 0 and cands(t=11) != 0
    assert cands(order=6) != 0 and cands(cap=6) != 0 and cands(V=8193) != 0 and cands(eos=100) != 0
    assert cands(alpha=float('nan')) != 0

    def seqs(n_hyp=4, T=8, order=3, eos=1):
        return lib.otr_ngram_score_seqs(p, 4, 1, order, 100, p, p, n_hyp, T, 1.0, 0.0, -1000.0, eos, p, None, None)
    assert seqs(n_hyp=-1) != 0 and seqs(T=-1) != 0 and seqs(order=0) != 0 and seqs(eos=-1) != 0
    assert b'ngram_score_seqs' in lib.otr_last_error_string()
    assert lib.otr_rescore_select_add(p, p, p, p, p, None, p, 1, 33, 4, 1, 0.3, 0.0, 0.0, 5.0, p, p, p, p, p, None) != 0
    assert lib.otr_rescore_select_add(p, p, p, p, p, None, None, 1, 4, 4, 5, 0.3, 0.0, 0.0, 5.0, p, p, p, p, p, None) != 0
