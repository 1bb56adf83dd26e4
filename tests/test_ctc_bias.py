"""CPU: phrase biasing in the CTC prefix beam search (otr_ctc_beam_search_bias, ops.ctc_prefix_beam_search_bias, CTCRecognizer
bias=..., SpeechToTextRecognizer bias_first_pass=True).  The restatement tests/ctc_prefix_bias_ref.py against brute force, against
the plain restatement and against the sequence score; the conditions the GPU tests (tests/test_gpu_ctc_bias.py) rely on, asserted
on the restatement alone; the refusals; the new entry in the header, the binding and both libraries."""
import ctypes as C
import math
import re
import types

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, ops
from opentransformer_amd.bias import PhraseBias
from tests import bias_ref
from tests import ctc_bias_cases as cases
from tests import ctc_prefix_bias_ref as bref
from tests import ctc_prefix_ref
from tests.bias_ref import RefBias
from tests.test_bias import HEADER, _model
from tests.test_ngram import c1_model, paths_by_string

NO_EOS = 99                                   # the brute-force cases have no EOS unit among their three
SMALL_SETS = {                                # V = 3: units 1 and 2; every set holds a phrase six frames cannot complete
    'nested': ([(1, 2), (1, 2, 1), (2, 2, 2, 2, 2, 2, 2)], [1.0, 0.5, 2.0]),
    'single': ([(2,), (1, 1), (1, 2, 1, 2, 1, 2, 1)], [0.5, 1.5, 3.0]),
    'shared': ([(2, 1, 2), (2, 1, 1), (1, 2), (2, 1, 2, 1, 2, 1, 2, 1)], [2.0, 1.0, 0.5, 1.5]),
}


def small_log_probs(seed, B=1):
    rng = np.random.default_rng(seed)
    return torch.log_softmax(torch.from_numpy(rng.normal(size=(B, 6, 3)) * 1.5), -1).numpy()


@pytest.mark.parametrize('name', sorted(SMALL_SETS))
def test_restated_search_is_exact_when_nothing_is_pruned(name):
    """V = 3, T = 6, K = 3, W = 32: up to frame 5 the beam holds every string the frames can spell (tests/test_ngram.py's argument), so
    nothing is pruned before the last selection and every live hypothesis scores ln sum(paths) + the phrase score of the string with
    its EOS step, i.e. what its completed phrases earned; the top hypothesis is the brute-force arg-max"""
    phrases, weights = SMALL_SETS[name]
    rb = RefBias(phrases, weights, 3, NO_EOS)
    for seed in (13, 14):
        lp = small_log_probs(seed)[0]
        every = paths_by_string(lp)
        total = {s: v + float(bias_ref.seq_score(rb, s, NO_EOS)) for s, v in every.items()}
        refunds = []
        hyps = bref.decode_one(lp, 6, 32, 3, rb, refunds=refunds)
        assert len(hyps) == 32 < len(every)
        for s, sc, ls, bs in hyps:
            assert ls == 0.0 and bs == float(bias_ref.seq_score(rb, s, NO_EOS)), s
            assert abs(sc - total[s]) <= 1e-9 * abs(sc) + 1e-9, (s, sc, total[s])
        assert hyps[0][0] == max(total, key=total.get)
        assert [h[1] for h in hyps] == sorted((h[1] for h in hyps), reverse=True)
        assert any(r > 0 for _, r in refunds[0])                                  # a match is open at the end
        assert all(s != max(phrases, key=len) for s in every)                     # ... and the long phrase is never completed


def test_the_restatement_shortcut_for_units_in_no_phrase_is_the_addend():
    p = cases.planted()
    rb = cases.planted_bias()[1]
    rng = np.random.default_rng(3)
    memo, foreign = {}, 0
    for q in range(400):
        ph = p['phrases'][int(rng.integers(len(p['phrases'])))]
        s = tuple(int(v) for v in rng.integers(2, cases.P_V, size=int(rng.integers(0, 20)))) + ph[:int(rng.integers(0, len(ph) + 1))]
        c = int(rng.integers(2, cases.P_V)) if q % 2 else int(ph[min(len(ph) - 1, int(rng.integers(0, 17)))])
        assert bref.phrase_addend(rb, s, c, memo) == float(rb.addend(s, c)), (s, c)
        foreign += c not in memo['units']
    assert foreign > 100


def test_zero_weights_give_the_plain_restatement():
    lp = cases.golden_log_probs().astype(np.float64)
    phrases, _ = cases.golden_phrases()
    rb = RefBias(list(phrases), [0.0] * len(phrases), cases.GOLDEN_V, cases.EOS)
    for b, n in enumerate(cases.GOLDEN_LENGTHS[1]):
        g0, g1 = [], []
        got = bref.decode_one(lp[b], n, 5, 40, rb, gaps=g0)
        assert [(s, sc) for s, sc, _, _ in got] == ctc_prefix_ref.decode_one(lp[b], n, 5, 40, gaps=g1) and g0 == g1
        assert all(ls == 0.0 and bs == 0.0 for _, _, ls, bs in got)


COMBOS = [(W, K, ng) for ng in (False, True) for W in cases.GOLDEN_WS for K in cases.GOLDEN_KS]


@pytest.mark.parametrize('W,K,with_ngram', COMBOS)
def test_golden_case_is_clear_and_its_bias_score_is_the_sequence_score(W, K, with_ngram):
    """every golden combination leaves >= 3 of 4 utterances clear of a near-tie (the GPU test's min_clear), and the bias score of every
    hypothesis is the summed addends of the string + EOS, exactly (dyadic weights)"""
    rb = cases.golden_bias()[1]
    for which in range(len(cases.GOLDEN_LENGTHS)):
        tokens, out_len, scores, lm_scores, bias_scores, gaps, _ = cases.golden_reference(W, K, with_ngram, which)
        assert cases.clear_count(gaps) >= 3, (which, gaps)
        for b in range(tokens.shape[0]):
            live = scores[b] > -math.inf
            assert (np.diff(scores[b][live]) <= 0).all()
            for r in np.flatnonzero(live):
                h = tokens[b, r, :out_len[b, r]].tolist()
                assert bias_scores[b, r] == float(bias_ref.seq_score(rb, h, cases.EOS)), (b, r, h)
            assert with_ngram or (lm_scores[b] == 0).all()


def test_golden_phrase_set_is_what_the_case_says():
    phrases, weights = cases.golden_phrases()
    pb, _ = cases.golden_bias()
    assert 50 <= len(phrases) <= 64 and set(weights) <= set(cases.WEIGHTS) and len(set(weights)) == len(cases.WEIGHTS)
    assert all(2 <= min(p) and max(p) < cases.GOLDEN_V and 1 <= len(p) <= 16 for p in phrases)
    assert max(len(p) for p in phrases) == 16 and pb.max_len == 16
    assert any(p != q and q[:len(p)] == p for p in phrases for q in phrases)                        # a prefix of another
    assert any(p != q and p[:2] == q[:2] and p[:3] != q[:3] and len(p) > 2 and len(q) > 2 for p in phrases for q in phrases)
    changed = sum(tuple(cases.golden_reference(W, K, ng, 0)[0][b, 0]) != tuple(cases.golden_plain(W, K, 0)[0][b, 0])
                  for W, K, ng in COMBOS if not ng for b in range(4))
    assert changed >= 9                                                                              # the phrases change 1-bests
    moved = sum([s for s, _ in rf] != [tuple(t[b, r, :n[b, r]].tolist()) for r in range(len(rf))]
                for W, K, ng in COMBOS for which in (0, 1)
                for t, n, _, _, _, _, refunds in [cases.golden_reference(W, K, ng, which)] for b, rf in enumerate(refunds))
    assert moved >= 10                                                                               # ... and refunds reorder beams


def test_planted_case_walks_every_path_of_the_chain_logic():
    """>= 4 of 5 utterances clear; a chain of depth 16, a fail-over from one phrase to another, a non-zero refund after the last frame
    and a beam that the refund reorders all occur in the restatement's final beams"""
    p = cases.planted()
    pb, rb = cases.planted_bias()
    assert 56 <= len(p['phrases']) <= 64 and pb.max_len == 16
    ids = {v for ph in p['phrases'] for v in ph}
    assert max(ids) > 4096 and sum(255 < v < 4096 for v in ids) > 20
    tokens, out_len, scores, _, bias_scores, gaps, refunds = cases.planted_reference()
    assert cases.clear_count(gaps) >= 4, gaps
    hyps = [[tuple(tokens[b, r, :out_len[b, r]].tolist()) for r in range(cases.P_W) if scores[b, r] > -math.inf] for b in range(cases.P_B)]
    depth = lambda h: max(len(rb.state(h[:l])) for l in range(len(h) + 1))                           # noqa: E731
    assert max(depth(h) for h in hyps[0]) == 16 and max(depth(h) for h in hyps[1]) == 15
    assert bias_scores[0, 0] == float(rb.psi_minus(p['named']['P16'])) and (bias_scores[1] == 0).all()    # completed / all refunded
    A, A2 = p['named']['A'], p['named']['A2']
    fail_over = [h for h in hyps[2] for l in range(len(h)) if rb.state(h[:l]) == A[:3] and rb.state(h[:l + 1]) == A2]
    assert fail_over and bias_scores[2, 0] > 0
    assert any(r > 0 for _, r in refunds[3]) and any(r == 0 for _, r in refunds[3])
    assert [s for s, _ in refunds[3]] != hyps[3] and sorted(s for s, _ in refunds[3]) == sorted(hyps[3])
    z = p['named']['Z'][0]
    assert any(h[:2] == (z, z) for h in hyps[4])                                                     # the doubled unit survives
    for b in range(cases.P_B):
        for r, h in enumerate(hyps[b]):
            assert bias_scores[b, r] == float(bias_ref.seq_score(rb, h, cases.EOS))


def test_a_hypothesis_is_brought_back():
    """utterance 0 of the golden case at W = 5, K = 40: the biased 5-best holds a hypothesis that the unbiased 5-best does not, and
    a phrase of the set pays for it"""
    which, b, W, K = cases.BROUGHT_BACK
    tokens, out_len, scores, _, bias_scores, gaps, _ = cases.golden_reference(W, K, False, which)
    pt, pl, _ = cases.golden_plain(W, K, which)
    assert gaps[b] > cases.GAP
    biased = {tuple(tokens[b, r, :out_len[b, r]].tolist()): bias_scores[b, r] for r in range(W)}
    plain = {tuple(pt[b, r, :pl[b, r]].tolist()) for r in range(W)}
    back = cases.BROUGHT_BACK_HYP
    assert back in biased and back not in plain and biased[back] > 0
    assert any(back[o:o + len(p)] == p for p in cases.golden_phrases()[0] for o in range(len(back)))


# ---------------------------------------------------------------- refusals, without a GPU
def test_the_entry_refuses_bad_arguments():
    lib = _lib.load()
    al, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    ws = lib.otr_ctc_beam_workspace_bytes(2, 8, 5)

    def search(W=5, K=40, blank=0, ws_bytes=ws, ngram=None, cap=0, probe=0, order=0, alpha=0.0, lm_scores=None, table=al, bcap=64,
               bprobe=2, max_len=4, bias_scores=al, tokens=al):
        return lib.otr_ctc_beam_search_bias(al, al, al, 2, 8, 100, K, blank, W, al, ws_bytes, tokens, al, al, ngram, cap, probe, order,
                                            alpha, 1.0, -1000.0, lm_scores, table, bcap, bprobe, max_len, bias_scores, None)
    for kw, word in ((dict(W=33), b'beam width'), (dict(W=0), b'beam width'), (dict(K=101), b'K='), (dict(blank=100), b'blank'),
                     (dict(ws_bytes=ws - 8), b'workspace'), (dict(tokens=None), b'null'), (dict(bias_scores=None), b'null'),
                     (dict(table=None), b'table'), (dict(table=odd), b'aligned'), (dict(bcap=48), b'capacity'), (dict(bcap=0), b'capacity'),
                     (dict(bprobe=0), b'max_probe'), (dict(bprobe=65), b'max_probe'), (dict(max_len=0), b'max_len'),
                     (dict(max_len=17), b'max_len'), (dict(lm_scores=al), b'lm_scores'),
                     (dict(ngram=al, cap=1024, probe=3, order=3), b'lm_scores'),
                     (dict(ngram=al, cap=1000, probe=3, order=3, lm_scores=al), b'power of two'),
                     (dict(ngram=al, cap=1024, probe=0, order=3, lm_scores=al), b'max_probe'),
                     (dict(ngram=al, cap=1024, probe=3, order=6, lm_scores=al), b'order'),
                     (dict(ngram=C.c_void_p(4096 + 16), cap=1024, probe=3, order=3, lm_scores=al), b'aligned'),
                     (dict(ngram=al, cap=1024, probe=3, order=3, lm_scores=al, alpha=float('nan')), b'numbers')):
        assert search(**kw) < 0, kw
        err = lib.otr_last_error_string()
        assert b'ctc_beam_search_bias' in err and word in err, (kw, err)


def test_the_op_refuses_before_any_launch():
    lp, ln = torch.zeros(1, 4, 12), torch.tensor([4])
    with pytest.raises(_lib.OtransHipError, match='PhraseBias'):
        ops.ctc_prefix_beam_search_bias(lp, ln, [[2, 3]])
    with pytest.raises(_lib.OtransHipError, match='PhraseBias'):
        ops.ctc_prefix_beam_search_bias(lp, ln, None)
    with pytest.raises(_lib.OtransHipError, match='100 units'):
        ops.ctc_prefix_beam_search_bias(lp, ln, PhraseBias([[2, 3]], 100))
    with pytest.raises(_lib.OtransHipError, match='blank'):
        ops.ctc_prefix_beam_search_bias(lp, ln, PhraseBias([[2, 3], [4, 0]], 12))
    with pytest.raises(_lib.OtransHipError, match='blank'):
        ops.ctc_prefix_beam_search_bias(lp, ln, PhraseBias([[2, 3]], 12), blank=3)
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):               # everything else is in order: it gets to the device check
        ops.ctc_prefix_beam_search_bias(lp, ln, PhraseBias([[2, 3]], 12))


def test_recognizers_refuse_and_accept(tmp_path):
    from opentransformer_amd.recognize import CTCRecognizer, SpeechToTextRecognizer, build_recognizer
    model = c1_model()
    idx2unit = {i: 'u%d' % i for i in range(100)}
    pb = PhraseBias([[2, 3]], 100)
    rec = CTCRecognizer(model, idx2unit=idx2unit, mode='beam', bias=pb)
    assert rec.bias is pb and CTCRecognizer(model, idx2unit=idx2unit, mode='beam').bias is None
    assert CTCRecognizer(model, idx2unit=idx2unit, mode='greedy', bias=pb).mode == 'greedy'          # ignored, as ngram_lm is
    for bad in ([[2, 3]], 'phrases.txt'):
        with pytest.raises(TypeError, match='PhraseBias'):
            CTCRecognizer(model, idx2unit=idx2unit, mode='beam', bias=bad)
    path = tmp_path / 'phrases.txt'
    path.write_text('u2 u3 u4\nu5 u6\t4.0\nu7 nope\n')
    args = types.SimpleNamespace(lm_weight=0.1, ngram_lm=None, beam_width=4, ngpu=1, mode='beam', alpha=0.3, beta=0.2,
                                 bias_phrases=str(path), bias_score=1.25)
    built = build_recognizer('ctc', model, None, args, idx2unit)
    assert isinstance(built.bias, PhraseBias) and built.bias.vocab_size == 100
    assert built.bias.phrases == [(2, 3, 4), (5, 6)] and built.bias.weights == [1.25, 4.0] and built.bias.skipped == [('u7 nope', ['nope'])]
    args.bias_phrases = pb
    assert build_recognizer('ctc', model, None, args, idx2unit).bias is pb
    del args.bias_phrases
    assert build_recognizer('ctc', model, None, args, idx2unit).bias is None
    # the two-pass decoder's first pass
    pb12 = PhraseBias([[2, 3]], 12)
    kw = dict(ctc_weight=0.3, beam_width=4)
    r = SpeechToTextRecognizer(_model(0.3), rescore=True, bias=pb12, bias_first_pass=True, **kw)
    assert r.bias_first_pass is True
    assert SpeechToTextRecognizer(_model(0.3), rescore=True, bias=pb12, **kw).bias_first_pass is False
    with pytest.raises(ValueError, match='bias_first_pass'):
        SpeechToTextRecognizer(_model(0.3), rescore=True, bias_first_pass=True, **kw)               # no phrases
    with pytest.raises(ValueError, match='bias_first_pass'):
        SpeechToTextRecognizer(_model(0.3), bias=pb12, bias_first_pass=True, **kw)                  # no second pass
    with pytest.raises(ValueError, match='bias_first_pass'):
        SpeechToTextRecognizer(_model(0.3), joint_ctc=True, bias=pb12, bias_first_pass=True, **kw)
    sargs = types.SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1,
                                  bias_phrases=pb12, rescore=True, bias_first_pass=True)
    assert build_recognizer('speech2text', _model(0.3), None, sargs, None).bias_first_pass is True
    del sargs.bias_first_pass
    assert build_recognizer('speech2text', _model(0.3), None, sargs, None).bias_first_pass is False


def test_the_entry_is_in_the_header_the_binding_and_both_libraries():
    header = open(HEADER).read()
    assert re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1) == '608' and _lib.OTR_ABI_VERSION == 608
    still = header[header.index('still 608'):header.index('#define OTR_ABI_VERSION')]
    name = 'otr_ctc_beam_search_bias'
    assert re.search(r'\b%s\(' % name, header) and name in still and len(_lib.SIGNATURES[name]) == 28
    proto = header[header.index('int32_t %s(' % name):]
    assert proto[:proto.index(';')].count(',') == 27
    for kind in ('bf16', 'fp16'):
        lib = _lib.load(kind)
        assert lib.otr_version() == 608 and getattr(lib, name) is not None
