"""CPU: the restatement tests/nbest_consensus_ref.py against tests/edit_distance_ref.py and against cases worked out by hand, the MBR
properties of the definition, evaluate.calibration, and the plumbing that needs no GPU (the header, the binding, the argument checks
of the wrappers and of the recognizers' constructors)."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, evaluate, ops
from tests import edit_distance_ref as ed
from tests import nbest_consensus_cases as cases
from tests import nbest_consensus_ref as ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'otrans_hip.h')


def counts_of(R, code):
    """(S, D, I) of an alignment's codes against a reference of R tokens"""
    m, s, i = code.count(ref.MATCH), code.count(ref.SUB), code.count(ref.INS)
    return s, R - m - s, i


@pytest.mark.parametrize('alphabet', [2, 4, 30])
def test_align_reproduces_the_counts_of_the_edit_distance(alphabet):
    rng = np.random.default_rng(alphabet)
    for _ in range(150):
        R, H = int(rng.integers(0, 14)), int(rng.integers(0, 14))
        r, h = rng.integers(0, alphabet, R).tolist(), rng.integers(0, alphabet, H).tolist()
        dist, code, pos = ref.align(r, h)
        want = ed.pair(r, h)
        assert (dist,) + counts_of(R, code) == tuple(want) == tuple(ed.pair_backtrace(r, h)), (r, h)
        assert len(code) == len(pos) == H
        aligned = [p for p in pos if p >= 0]
        assert aligned == sorted(set(aligned)) and all(0 <= p < R for p in aligned)         # monotone, one reference token each
        for k in range(H):
            assert (code[k] == ref.INS) == (pos[k] < 0)
            if pos[k] >= 0:
                assert (code[k] == ref.MATCH) == (r[pos[k]] == h[k])


def test_align_at_the_chunk_edges_against_the_row_form():
    r, rl, h, hl = cases.align_grid()
    for b in range(0, len(rl), 7):
        rr, hh = r[b, :rl[b]].tolist(), h[b, 0, :hl[b, 0]].tolist()
        dist, code, _ = ref.align(rr, hh)
        assert (dist,) + counts_of(len(rr), code) == ed.pair_fast(rr, hh)


def test_align_edges():
    assert ref.align([], []) == (0, [], [])
    assert ref.align([1, 2], []) == (2, [], [])
    assert ref.align([], [1, 2]) == (2, [2, 2], [-1, -1])
    assert ref.align([1, 2, 3], [1, 4, 3]) == (1, [0, 1, 0], [0, 1, 2])
    # the tie rule: [1, 1] against the reference [1] is an insertion and a match; from (1, 2) the diagonal (a match, D[0][1] + 0 ==
    # D[1][2]) comes before the cell to the left, so the LAST token is the match
    assert ref.align([1], [1, 1]) == (1, [2, 0], [-1, 0])
    dist, code, pos = ref.align_batch(np.array([[1, 2, 3]]), [3], np.array([[[1, 9, 3, 7], [1, 2, 3, 0]]]), [[2, 9]], eos=9)
    assert dist.tolist() == [[2, -1]] and code.tolist() == [[[0, -1, -1, -1], [-1] * 4]] and pos.tolist() == [[[0, -1, -1, -1], [-1] * 4]]


@pytest.mark.parametrize('case', cases.HAND, ids=[c['name'] for c in cases.HAND])
def test_hand_made_cases(case):
    tokens, lengths, scores = cases.hand_arrays(case)
    post, risk, best, conf, live = ref.consensus(tokens, lengths, scores, case['scale'])
    tol = 1e-7              # the scores are float32: ln 3 is rounded at 2^-24 relative, and so is the posterior made of it
    assert best.tolist() == [case['best']]
    assert live[0].tolist() == [math.isfinite(s) for s in case['scores']]
    if case['post'] is not None:
        np.testing.assert_allclose(post[0], case['post'], rtol=0, atol=tol)
    if case['risk'] is not None:
        np.testing.assert_allclose(risk[0], case['risk'], rtol=0, atol=tol)
    if case['conf'] is not None:
        for n, c in enumerate(case['conf']):
            np.testing.assert_allclose(conf[0, n, :len(c)], c, rtol=0, atol=tol)
            assert (conf[0, n, len(case['tokens'][n]):] == 0).all()
    assert abs(post[0].sum() - (1.0 if live.any() else 0.0)) < 1e-12


def test_a_length_outside_the_width_and_eos():
    tokens = np.array([[[1, 2, 3], [1, 2, 4], [1, 5, 3]]])
    post, risk, best, conf, live = ref.consensus(tokens, [[3, 4, -1]], [[0.0, 5.0, 5.0]])
    assert live.tolist() == [[True, False, False]] and best.tolist() == [0] and post.tolist() == [[1.0, 0.0, 0.0]]
    assert risk[0, 0] == 0 and np.isinf(risk[0, 1:]).all() and (conf[0, 1:] == 0).all()
    # eos cuts [1, 2, 4] to [1]: slot 0 against it is a match and two insertions
    post, risk, best, conf, _ = ref.consensus(np.array([[[1, 2, 3], [1, 0, 4]]]), None, None, eos=0)
    assert risk.tolist() == [[1.0, 1.0]] and conf.tolist() == [[[1.0, 0.5, 0.5], [1.0, 0.0, 0.0]]]


def test_mbr_properties():
    for name, B, N, lens, scale, seed in cases.CONSENSUS[:3]:
        tokens, lengths, scores = cases.consensus_inputs(B, N, tuple(min(n, 20) for n in lens), seed)
        post, risk, best, conf, live = ref.consensus(tokens, lengths, scores, scale)
        for b in range(B):
            if N == 1:
                assert best[b] == 0 and risk[b, 0] == 0 and post[b, 0] == 1
            assert (conf[b] <= 1 + 1e-12).all() and (conf[b] >= 0).all()
            for n in range(N):
                if live[b, n]:                                              # a token always agrees with its own hypothesis
                    assert (conf[b, n, :lengths[b, n]] >= post[b, n] - 1e-15).all()
    # scale -> large: the posterior is one-hot and the arg-max score has risk 0, the others (different strings) more
    tokens, lengths, scores = cases.consensus_inputs(4, 6, (5, 6, 7, 8), 11, dead=False)
    for b in range(4):
        assert len({tuple(tokens[b, n, :lengths[b, n]]) for n in range(6)}) == 6
    _, risk, best, _, _ = ref.consensus(tokens, lengths, scores, scale=1e4)
    assert best.tolist() == scores.argmax(-1).tolist()
    # scale 0: the uniform posterior, whatever the scores
    post, _, _, _, _ = ref.consensus(tokens, lengths, scores, scale=0.0)
    assert (post == 1 / 6).all()


def test_the_generated_cases_are_clear_of_near_ties():
    """the same assertion the GPU test makes before it compares `best`, here on the cheap cases"""
    for name, B, N, lens, scale, seed in cases.CONSENSUS[:4]:
        tokens, lengths, scores = cases.consensus_inputs(B, N, lens, seed)
        _, risk, _, _, live = ref.consensus(tokens, lengths, scores, scale)
        assert cases.clear_of_near_ties(risk, scores, live), name
    assert not cases.clear_of_near_ties(np.array([[1.0, 1.0005]]), None, np.array([[True, True]]))
    assert cases.clear_of_near_ties(np.array([[1.0, 1.0, 1.0005]]), None, np.array([[True, True, True]]))


def test_calibration_by_hand():
    c = cases.CALIBRATION
    nce, ece = ref.calibration(c['conf'], c['correct'])
    assert abs(nce - c['nce']) < 1e-12 and abs(ece - c['ece']) < 1e-12
    got = evaluate.calibration(torch.tensor(c['conf']), torch.tensor(c['correct']))
    assert got['tokens'] == 4 and abs(got['nce'] - c['nce']) < 1e-6 and abs(got['ece'] - c['ece']) < 1e-6      # f32 confidences
    # a mask leaves elements out; bool outcomes; any shape
    conf = torch.tensor([[0.9, 0.8, 0.11], [0.3, 0.6, 0.99]])
    correct = torch.tensor([[True, True, False], [False, False, False]])
    mask = torch.tensor([[True, True, False], [True, True, False]])
    got2 = evaluate.calibration(conf, correct, mask)
    assert got2['tokens'] == 4 and abs(got2['nce'] - got['nce']) < 1e-12 and abs(got2['ece'] - got['ece']) < 1e-12
    # perfect and confident: NCE -> 1, ECE -> 0; every outcome the same: NCE undefined; nothing: both undefined
    sure = evaluate.calibration(torch.tensor([1.0, 0.0, 1.0, 0.0]), torch.tensor([1, 0, 1, 0]))
    assert sure['nce'] > 0.9999 and sure['ece'] == 0
    assert math.isnan(evaluate.calibration(torch.tensor([0.5, 0.7]), torch.tensor([1, 1]))['nce'])
    none = evaluate.calibration(torch.zeros(0), torch.zeros(0))
    assert none['tokens'] == 0 and math.isnan(none['nce']) and math.isnan(none['ece'])
    rng = np.random.default_rng(0)
    conf, correct = rng.random(500).astype(np.float32), rng.integers(0, 2, 500)
    nce, ece = ref.calibration(conf, correct)
    got = evaluate.calibration(torch.from_numpy(conf), torch.from_numpy(correct))
    assert abs(got['nce'] - nce) < 1e-9 and abs(got['ece'] - ece) < 1e-9


def test_the_entries_are_in_the_header_the_binding_and_both_libraries():
    header = open(HEADER).read()
    assert int(re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1)) == _lib.OTR_ABI_VERSION
    assert int(re.search(r'#define OTR_NBEST_MAX_LEN (\d+)', header).group(1)) == ops.NBEST_MAX_LEN == cases.MAX_LEN >= 256
    for name in ('otr_edit_align', 'otr_nbest_consensus'):
        proto = header[header.index('int32_t %s(' % name):]
        assert proto[:proto.index(';')].count(',') + 1 == len(_lib.SIGNATURES[name])
        for kind in ('bf16', 'fp16'):
            assert getattr(_lib.load(kind), name) is not None


def test_the_wrappers_refuse_bad_arguments_before_any_launch():
    t = torch.zeros((2, 3, 5), dtype=torch.int64)
    wide = torch.zeros((1, 1, ops.NBEST_MAX_LEN + 1), dtype=torch.int64)
    with pytest.raises(ValueError, match='at most 256'):
        ops.nbest_consensus(wide)
    with pytest.raises(ValueError, match='at most 256'):
        ops.edit_align(torch.zeros((1, 4), dtype=torch.int64), torch.tensor([4]), wide)
    with pytest.raises(ValueError, match='at most 256'):
        ops.edit_align(wide[0], torch.tensor([4]), torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='1 .. 32'):
        ops.nbest_consensus(torch.zeros((1, 33, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='1 .. 32'):
        ops.edit_align(torch.zeros((1, 4), dtype=torch.int64), torch.tensor([4]), torch.zeros((1, 33, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='finite'):
        ops.nbest_consensus(t, scale=float('inf'))
    with pytest.raises(ValueError):
        ops.nbest_consensus(t[0])
    with pytest.raises(ValueError):
        ops.edit_align(torch.zeros((3, 4), dtype=torch.int64), torch.tensor([4] * 3), t)
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):
        ops.nbest_consensus(t)
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):
        ops.edit_align(torch.zeros((2, 4), dtype=torch.int64), torch.tensor([4, 4]), t)


def test_the_recognizers_take_mbr_and_refuse_what_they_cannot_do():
    import opentransformer_amd as ota
    from opentransformer_amd import synthetic as syn
    from opentransformer_amd.recognize import CTCRecognizer, SpeechToTextRecognizer, build_recognizer
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    rec = SpeechToTextRecognizer(model)
    assert rec.mbr is False and rec.mbr_scale == 1.0
    rec = SpeechToTextRecognizer(model, mbr=True, mbr_scale=0.5, beam_width=32)
    assert rec.mbr is True and rec.mbr_scale == 0.5
    with pytest.raises(ValueError, match='beam_width'):
        SpeechToTextRecognizer(model, mbr=True, beam_width=33)
    with pytest.raises(ValueError, match='finite'):
        SpeechToTextRecognizer(model, mbr_scale=float('nan'))
    assert CTCRecognizer(model, mode='beam', mbr=True, mbr_scale=2.0).mbr_scale == 2.0 and CTCRecognizer(model).mbr is False
    with pytest.raises(ValueError, match='beam'):
        CTCRecognizer(model, mode='greedy', mbr=True)
    with pytest.raises(ValueError, match='beam'):
        CTCRecognizer(model, mode='greedy').recognize_with_confidence(None, None)
    with pytest.raises(ValueError, match='beam'):
        CTCRecognizer(model, mode='greedy').recognize_tokens_with_confidence(None, None)
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=5, nbest=2, max_len=10, penalty=0, lamda=5, ngpu=1, ngram_lm=None,
                           mode='beam', alpha=0.1, beta=0.0)
    for kind in ('speech2text', 'ctc'):
        assert build_recognizer(kind, model, None, args, None).mbr is False
        args2 = SimpleNamespace(mbr=True, mbr_scale=0.7, **vars(args))
        rec = build_recognizer(kind, model, None, args2, None)
        assert rec.mbr is True and rec.mbr_scale == 0.7
