"""GPU (-m gpu): phrase biasing fused into the CTC prefix beam search (otr_ctc_beam_search_bias, ops.ctc_prefix_beam_search_bias,
CTCRecognizer bias=..., SpeechToTextRecognizer bias_first_pass=True) against tests/ctc_prefix_bias_ref.py, brute force, the plain
and the n-gram searches and the sequence kernel.  tests/test_ctc_bias.py asserts, without a GPU, that every input compared here
leaves at least `min_clear` utterances clear of a near-tie and walks the paths its name promises."""
import ctypes as C
import io
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, ops
from opentransformer_amd.bias import PhraseBias
from opentransformer_amd.ngram import NGramLM
from tests import ctc_bias_cases as cases
from tests import ngram_cases
from tests.bias_ref import RefBias, seq_score
from tests.ngram_ref import RefLM, make_lm
from tests.test_ctc_bias import COMBOS, NO_EOS, SMALL_SETS, small_log_probs
from tests.test_gpu_ctc_beam import hyps_of, load_c1
from tests.test_gpu_ctc_ngram import peaky
from tests.test_ngram import paths_by_string

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def run(lp, lengths, pb, W, K, lm=None, alpha=0.0, beta=0.0, blank=0):
    """the op's outputs as numpy: (tokens, out_len, scores, lm_scores or None, bias_scores)"""
    out = ops.ctc_prefix_beam_search_bias(torch.from_numpy(lp).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV), pb, lm,
                                          alpha, beta, beam_width=W, cutoff_top_n=K, blank=blank)
    out = tuple(t.cpu().numpy() for t in out)
    return out if lm is not None else out[:3] + (None, out[3])


def check_against_reference(got, want, W, min_clear):
    """tests/test_gpu_ctc_ngram.py's comparison with bias_scores added: wherever the restatement's W/W+1 gap exceeds GAP at every
    frame the beams hold the same strings, scores, lm_scores and bias_scores within 1e-5 relative + 1e-6, and the order is the
    restatement's except across gaps <= GAP"""
    tokens, out_len, scores, lm_scores, bias_scores = got
    rt, rl, rs, rlm, rbs, gaps, _ = want
    B, _, T = rt.shape
    assert tokens.shape == (B, W, T) and out_len.shape == (B, W) and scores.shape == (B, W) and bias_scores.shape == (B, W)
    clear = 0
    for b in range(B):
        s = scores[b]
        live = s > -math.inf
        assert (np.diff(s[live]) <= 0).all(), b
        assert not live[live.sum():].any()
        assert (out_len[b][~live] == 0).all() and (tokens[b][~live] == -1).all() and (bias_scores[b][~live] == 0).all()
        assert lm_scores is None or (lm_scores[b][~live] == 0).all()
        for r in range(W):
            assert (tokens[b, r, out_len[b, r]:] == -1).all() and (tokens[b, r, :out_len[b, r]] >= 0).all()
        if gaps[b] <= cases.GAP:
            continue
        clear += 1
        g_s, w_s = hyps_of(tokens, out_len, scores, b), hyps_of(rt, rl, rs, b)
        assert set(g_s) == set(w_s), (b, W)
        for r in range(W):
            if rs[b, r] == -math.inf:
                continue
            h = tuple(rt[b, r, :rl[b, r]].tolist())
            q = [x for x in range(W) if live[x] and tuple(tokens[b, x, :out_len[b, x]].tolist()) == h]
            assert len(q) == 1, (b, h)
            assert abs(scores[b, q[0]] - rs[b, r]) <= 1e-5 * abs(rs[b, r]) + 1e-6, (b, h, scores[b, q[0]], rs[b, r])
            assert abs(bias_scores[b, q[0]] - rbs[b, r]) <= 1e-5 * abs(rbs[b, r]) + 1e-6, (b, h, bias_scores[b, q[0]], rbs[b, r])
            if lm_scores is not None:
                assert abs(lm_scores[b, q[0]] - rlm[b, r]) <= 1e-5 * abs(rlm[b, r]) + 1e-6, (b, h, lm_scores[b, q[0]], rlm[b, r])
        order_ok = all(abs(rs[b, r] - rs[b, r + 1]) <= cases.GAP or tuple(tokens[b, r, :out_len[b, r]]) == tuple(rt[b, r, :rl[b, r]])
                       for r in range(int(live.sum()) - 1))
        assert order_ok, b
    assert clear >= min_clear, (clear, gaps)


def same_as_the_sequence_kernel(pb, got, eos=cases.EOS):
    """dyadic weights: bias_scores is ops.bias_score_sequences of the same hypotheses, bit for bit"""
    tokens, out_len, _, _, bias_scores = got
    seq = ops.bias_score_sequences(pb, torch.from_numpy(tokens).to(DEV), torch.from_numpy(out_len).to(DEV), eos=eos)
    assert torch.equal(seq.cpu(), torch.from_numpy(bias_scores))


@pytest.mark.parametrize('W,K,with_ngram', COMBOS)
def test_search_matches_restatement_on_reference_log_probs(W, K, with_ngram):
    """the CTC head's log-probs of tests/golden/c1_decode.npz, full and ragged lengths, about 60 phrases; with the n-gram of
    tests/ngram_cases.py (order 3, alpha 0.5, beta 1.0) and without"""
    lp = cases.golden_log_probs()
    pb = cases.golden_bias()[0]
    lm = ngram_cases.golden_lm(3)[0] if with_ngram else None
    for which, lengths in enumerate(cases.GOLDEN_LENGTHS):
        got = run(lp, lengths, pb, W, K, lm, cases.ALPHA if with_ngram else 0.0, cases.BETA if with_ngram else 0.0)
        check_against_reference(got, cases.golden_reference(W, K, with_ngram, which), W, min_clear=3)
        same_as_the_sequence_kernel(pb, got)


def test_planted_case_matches_the_restatement():
    """B = 5, T = 64, V = 4233, W 10, K 40: a 16-id phrase completed, 15 of its ids refunded, a fail-over between phrases, an
    utterance that ends inside a phrase and a doubled unit in front of a phrase (tests/ctc_bias_cases.planted)"""
    p = cases.planted()
    pb = cases.planted_bias()[0]
    got = run(p['lp'], p['lengths'], pb, cases.P_W, cases.P_K)
    check_against_reference(got, cases.planted_reference(), cases.P_W, min_clear=4)
    same_as_the_sequence_kernel(pb, got)


def test_zero_weights_give_the_other_searches_bit_for_bit():
    lp = torch.from_numpy(peaky(4, 5, 120, 4233)).to(DEV)
    ln = torch.tensor([120, 77, 1, 0, 119], dtype=torch.int32, device=DEV)
    phrases = cases.planted()['phrases'] + [(int(v),) for v in range(2, 4233, 7)]      # every seventh unit too: matches do happen
    pb = PhraseBias(phrases, 4233, weights=[0.0] * len(phrases))
    kw = dict(beam_width=10, cutoff_top_n=40)
    plain = ops.ctc_prefix_beam_search(lp, ln, **kw)
    fused = ops.ctc_prefix_beam_search_bias(lp, ln, pb, **kw)
    assert len(fused) == 4
    for a, b in zip(plain, fused[:3]):
        assert torch.equal(a, b)
    assert (fused[3] == 0).all() and int(fused[1].max()) > 20
    lm = ngram_cases.size_lm()[0]
    with_lm = ops.ctc_prefix_beam_search_lm(lp, ln, lm, ngram_cases.ALPHA, ngram_cases.BETA, **kw)
    both = ops.ctc_prefix_beam_search_bias(lp, ln, pb, lm, ngram_cases.ALPHA, ngram_cases.BETA, **kw)
    assert len(both) == 5
    for a, b in zip(with_lm, both[:4]):
        assert torch.equal(a, b)
    assert (both[4] == 0).all() and not torch.equal(with_lm[2], plain[2])


def two_frames(pa, pb_, V=5, rest=1e-7):
    """two frames in which the blank has probability 0.5, units 2 and 3 have pa and pb_ = 0.5 - pa, and everything else next to
    nothing: the one-unit strings [2] and [3] (p^2 + p: the paths uu, u-, -u) outweigh every two-unit string, boosted or not"""
    p = np.full((1, 2, V), rest)
    p[0, :, 0], p[0, :, 2], p[0, :, 3] = 0.5, pa, pb_
    return np.log(p / p.sum(-1, keepdims=True)).astype(np.float32)


P_TENTH, P_HALF = 0.26041160515881245, 0.3014570564360813       # pa with ln((pa^2 + pa) / (pb^2 + pb)) = 0.1 / 0.5 at pb = 0.5 - pa


def test_the_phrase_decides():
    """unit a = 2 beats unit b = 3 by 0.1 nat over two frames; the phrase (b) at weight 1 makes [b] the 1-best, bias_scores 1"""
    lp = two_frames(P_TENTH, 0.5 - P_TENTH)
    t0, l0, s0 = (t.cpu().numpy() for t in ops.ctc_prefix_beam_search(torch.from_numpy(lp).to(DEV), torch.tensor([2], device=DEV),
                                                                      beam_width=4, cutoff_top_n=5))
    plain = hyps_of(t0, l0, s0, 0)
    assert abs(plain[(2,)] - plain[(3,)] - 0.1) < 1e-3 and t0[0, 0, :l0[0, 0]].tolist() == [2]
    tokens, out_len, scores, _, bias_scores = run(lp, [2], PhraseBias([(3,)], 5, weights=[1.0]), 4, 5)
    assert tokens[0, 0, :out_len[0, 0]].tolist() == [3] and bias_scores[0, 0] == 1.0
    got = hyps_of(tokens, out_len, scores, 0)
    assert abs(got[(3,)] - (plain[(3,)] + 1.0)) <= 1e-5 and abs(got[(2,)] - plain[(2,)]) <= 1e-6


def test_the_refund_decides():
    """b = 3 beats a = 2 by 0.5 nat; the phrase (a, c) at weight 2 lifts [a] above [b] inside the search, but c = 4 is never among the
    K = 4 candidates: the match stays open, is refunded after the last frame, and [b] is the 1-best again -- [a] with its
    unbiased score and a bias score of 0"""
    lp = two_frames(0.5 - P_HALF, P_HALF)
    lp[0, :, 4] -= 5.0                                                                     # c: the least likely unit of every frame
    x, ln = torch.from_numpy(lp).to(DEV), torch.tensor([2], device=DEV)
    t0, l0, s0 = (t.cpu().numpy() for t in ops.ctc_prefix_beam_search(x, ln, beam_width=4, cutoff_top_n=4))
    plain = hyps_of(t0, l0, s0, 0)
    assert abs(plain[(3,)] - plain[(2,)] - 0.5) < 1e-3 and not any(4 in h for h in plain)
    tokens, out_len, scores, _, bias_scores = run(lp, [2], PhraseBias([(2, 4)], 5, weights=[2.0]), 4, 4)
    got = hyps_of(tokens, out_len, scores, 0)
    assert tokens[0, 0, :out_len[0, 0]].tolist() == [3]
    r = [tuple(tokens[0, q, :out_len[0, q]].tolist()) for q in range(4)].index((2,))
    assert bias_scores[0, r] == 0.0 and abs(got[(2,)] - plain[(2,)]) <= 1e-5 * abs(plain[(2,)]) + 1e-6
    assert (3,) in got and abs(got[(3,)] - plain[(3,)]) <= 1e-5 * abs(plain[(3,)]) + 1e-6


@pytest.mark.parametrize('with_ngram', [False, True])
@pytest.mark.parametrize('name', sorted(SMALL_SETS))
def test_exhaustive_on_the_device(name, with_ngram):
    """V = 3, T = 6, W = 32, K = 3: nothing is pruned before the last selection, so every live hypothesis carries the brute-force
    score ln sum(paths) + the phrase score of the string (+ the n-gram's), bias_scores is that phrase score exactly, and
    scores - lm_scores - bias_scores is the unfused acoustic score within 1e-5"""
    phrases, weights = SMALL_SETS[name]
    pb, rb = PhraseBias(phrases, 3, weights=weights, eos_unit=0), RefBias(phrases, weights, 3, NO_EOS)
    lp = np.concatenate([small_log_probs(13), small_log_probs(14), small_log_probs(15), small_log_probs(16)]).astype(np.float32)
    lengths = [6, 6, 5, 4]
    lm, ref_lm, alpha, beta = None, None, 0.0, 0.0
    if with_ngram:
        text, grams, idx2unit = make_lm(2, 3, 3, (4, 6))
        lm, ref_lm, alpha, beta = NGramLM.from_arpa(io.StringIO(text), idx2unit), RefLM(grams, 3, 3), 0.6, 0.3
    tokens, out_len, scores, lm_scores, bias_scores = run(lp, lengths, pb, 32, 3, lm, alpha, beta)
    refunded = 0
    for b, n in enumerate(lengths):
        every = paths_by_string(lp[b, :n].astype(np.float64))
        ng = {s: (alpha * ref_lm.score(s) + beta * len(s)) if with_ngram else 0.0 for s in every}
        ph = {s: float(seq_score(rb, s, NO_EOS)) for s in every}
        total = {s: every[s] + ng[s] + ph[s] for s in every}
        got = hyps_of(tokens, out_len, scores, b)
        assert len(got) == min(32, len(every))
        best = sorted(total, key=total.get, reverse=True)
        assert total[best[0]] - total[best[1]] <= cases.GAP or tuple(tokens[b, 0, :out_len[b, 0]]) == best[0]
        for r in range(32):
            if scores[b, r] == -math.inf:
                continue
            s = tuple(tokens[b, r, :out_len[b, r]].tolist())
            assert bias_scores[b, r] == ph[s], (b, s)
            assert abs(scores[b, r] - total[s]) <= 1e-5 * abs(total[s]) + 1e-6, (b, s, scores[b, r], total[s])
            lm_part = lm_scores[b, r] if with_ngram else 0.0
            assert abs(lm_part - ng[s]) <= 1e-5 * abs(ng[s]) + 1e-6
            assert abs((scores[b, r] - lm_part - bias_scores[b, r]) - every[s]) <= 1e-5, (b, s)
            refunded += float(rb.psi(rb.state(s))) > 0
    assert refunded > 10


def test_deterministic_and_capturable():
    """two runs give equal bits; a captured graph (workspace passed, tables uploaded beforehand) replays to the eager outputs on
    both inputs"""
    p = cases.planted()
    pb = cases.planted_bias()[0].to(DEV)
    lm = ngram_cases.size_lm()[0].to(DEV)
    lp1 = p['lp']
    lp2 = np.ascontiguousarray(lp1[::-1])
    x = torch.from_numpy(lp1).to(DEV)
    ln = torch.tensor(p['lengths'], dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.load().otr_ctc_beam_workspace_bytes(cases.P_B, cases.P_T, cases.P_W) // 8, dtype=torch.int64, device=DEV)
    for ngram in (None, lm):
        call = lambda: ops.ctc_prefix_beam_search_bias(x, ln, pb, ngram, 0.5, 1.0, beam_width=cases.P_W, cutoff_top_n=cases.P_K,   # noqa: E731
                                                       workspace=ws)
        eager1 = [t.clone() for t in call()]
        again = call()
        for a, b in zip(eager1, again):
            assert torch.equal(a, b)
        x.copy_(torch.from_numpy(lp2))
        eager2 = [t.clone() for t in call()]
        assert not torch.equal(eager1[2], eager2[2])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            out = call()
        for lp, want in ((lp1, eager1), (lp2, eager2), (lp1, eager1)):
            x.copy_(torch.from_numpy(lp))
            g.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, want):
                assert torch.equal(a, b)


@pytest.mark.parametrize('with_ngram', [False, True])
def test_nothing_is_written_behind_the_outputs(with_ngram):
    """the entry called on output buffers with a guard row behind each: the guards keep their bits, the rows in front are the op's"""
    p = cases.planted()
    pb = cases.planted_bias()[0]
    lm = ngram_cases.size_lm()[0] if with_ngram else None
    B, T, V, W, K = cases.P_B, cases.P_T, cases.P_V, cases.P_W, cases.P_K
    x = torch.from_numpy(p['lp']).to(DEV)
    ln = torch.tensor(p['lengths'], dtype=torch.int32, device=DEV)
    want = ops.ctc_prefix_beam_search_bias(x, ln, pb, lm, 0.5, 1.0, beam_width=W, cutoff_top_n=K)
    lib = _lib.load()
    top_lp = torch.empty((B * T, K), dtype=torch.float32, device=DEV)
    top_tok = torch.empty((B * T, K), dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.otr_ctc_beam_workspace_bytes(B, T, W) // 8, dtype=torch.int64, device=DEV)
    tokens = torch.full((B + 1, W, T), 77, dtype=torch.int64, device=DEV)
    out_len = torch.full((B + 1, W), 77, dtype=torch.int32, device=DEV)
    scores, lm_scores, bias_scores = (torch.full((B + 1, W), 77.0, dtype=torch.float32, device=DEV) for _ in range(3))
    ptr = lambda t: C.c_void_p(t.data_ptr())                                                          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.otr_ctc_topk(ptr(x), V, ptr(ln), B, T, V, K, ptr(top_lp), ptr(top_tok), stream), 'otr_ctc_topk')
    ng = (ptr(lm.device_table(x.device)), lm.capacity, lm.max_probe, lm.order, 0.5, 1.0, lm.oov_score, ptr(lm_scores)) if with_ngram \
        else (None, 0, 0, 0, 0.0, 0.0, 0.0, None)
    _lib.check(lib.otr_ctc_beam_search_bias(ptr(top_lp), ptr(top_tok), ptr(ln), B, T, V, K, 0, W, ptr(ws), ws.numel() * 8, ptr(tokens),
                                            ptr(out_len), ptr(scores), *ng, ptr(pb.device_table(x.device)), pb.capacity, pb.max_probe,
                                            pb.max_len, ptr(bias_scores), stream), 'otr_ctc_beam_search_bias')
    torch.cuda.synchronize()
    got = (tokens, out_len, scores) + ((lm_scores,) if with_ngram else ()) + (bias_scores,)
    for a, b in zip(got, want):
        assert torch.equal(a[:B], b) and (a[B] == 77).all()
    assert with_ngram or (lm_scores == 77.0).all()


def test_ctc_recognizer_with_phrases(golden):
    """CTCRecognizer(mode='beam', bias=pb): recognize is translate of the fused op's 1-best on the log-probs the assistor produced in
    the same call, differs from the unbiased text, and recognize_with_times spells it; the same with ngram_lm too"""
    from opentransformer_amd.recognize import CTCRecognizer
    g = golden('c1_decode.npz')
    try:
        model = load_c1(g, 'fp32')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        seen = []
        inference = model.assistor.inference

        def recording(memory, memory_mask):
            out = inference(memory, memory_mask)
            seen.append(out)
            return out
        model.assistor.inference = recording
        pb = cases.golden_bias()[0]
        idx2unit = {i: str(i) for i in range(100)}
        for lm in (None, ngram_cases.golden_lm(3)[0]):
            kw = dict(idx2unit=idx2unit, mode='beam', beam_width=5, ngram_lm=lm, alpha=0.5, beta=1.0)
            rec = CTCRecognizer(model, bias=pb, **kw)
            del seen[:]
            texts = rec.recognize(x, m)
            lp, ln = seen[0]
            out = ops.ctc_prefix_beam_search_bias(lp, ln, pb, lm, 0.5, 1.0, beam_width=5, cutoff_top_n=40)
            tokens, out_len = out[0], out[1]
            assert texts == rec.translate([tokens[b, 0, :int(out_len[b, 0])].tolist() for b in range(4)])
            assert float(out[-1][:, 0].abs().sum()) > 0
            assert texts != CTCRecognizer(model, **kw).recognize(x, m)
            tk, tl, ts = rec.recognize_tokens(x, m)
            assert torch.equal(tk, tokens[:, :1]) and torch.equal(ts, out[2][:, :1])
            texts2, spans = rec.recognize_with_times(x, m)
            assert texts2 == texts
            for text, items in zip(texts, spans):
                assert ' '.join(u for u, _, _, _ in items) == text or [u for u, _, _, _ in items] == text.split()
                assert all(0 <= a < b <= 35 for _, a, b, _ in items)
    finally:
        ops.set_compute_dtype('bf16')


def test_two_pass_decoder_with_a_biased_first_pass(golden):
    """SpeechToTextRecognizer(rescore=True, bias=pb, bias_first_pass=True) on the C1 model in fp32: res['beam'] is the biased op's
    output, res['ctc'] its acoustic part, res['bias'] the sequence score; the hypothesis tests/test_ctc_bias.py shows to be brought
    back reaches the n-best and does not with bias_first_pass=False, whose pass is the parent's: the unbiased beam, re-ranked with
    the phrase score"""
    from tests.test_gpu_rescore import _arr, _head, _load, _rec
    try:
        _, model, _, _, x, m = _load(golden, 'fp32', False)
        pb = cases.golden_bias()[0]
        which, b0, W, K = cases.BROUGHT_BACK
        lam = 0.3
        kw = dict(beam_width=W, nbest=W, max_len=40, ctc_weight=lam, cutoff_top_n=K)
        first = _rec(model, None, bias=pb, bias_first_pass=True, **kw)
        mem, mm, lp, ln = _head(first, x, m)
        assert ln.tolist() == cases.LENGTH_SETS[which]
        with torch.no_grad():
            res = first.rescore_pass(mem, mm, lp, ln)
            tokens, out_len, scores, bias_scores = ops.ctc_prefix_beam_search_bias(lp, ln, pb, beam_width=W, cutoff_top_n=K)
            for a, b in zip(res['beam'], (tokens, out_len, scores)):
                assert torch.equal(a, b)
            assert torch.equal(res['ctc'], scores - bias_scores)
            seq = ops.bias_score_sequences(pb, tokens, out_len)
            assert torch.equal(res['bias'], seq) and torch.equal(seq, bias_scores) and float(seq.abs().sum()) > 0
            live = torch.isfinite(res['total'])
            want = (1.0 - lam) * res['att'] + lam * res['ctc'] + seq
            assert live.sum() >= 12 and torch.allclose(res['total'][live], want[live], rtol=1e-6, atol=1e-6)
            assert cases.BROUGHT_BACK_HYP in _arr(res)[b0]
            # the default: the parent's pass, assembled from the unbiased search, the unbiased pass's own terms and the sequence score
            default = _rec(model, None, bias=pb, **kw)
            assert default.bias_first_pass is False
            res_d = default.rescore_pass(mem, mm, lp, ln)
            res_0 = _rec(model, None, **kw).rescore_pass(mem, mm, lp, ln)
            plain = ops.ctc_prefix_beam_search(lp, ln, beam_width=W, cutoff_top_n=K)
            for a, b, c in zip(res_d['beam'], plain, res_0['beam']):
                assert torch.equal(a, b) and torch.equal(a, c)
            assert torch.equal(res_d['ctc'], plain[2]) and torch.equal(res_d['att'], res_0['att'])
            seq_d = ops.bias_score_sequences(pb, plain[0], plain[1])
            assert torch.equal(res_d['bias'], seq_d)
            live = torch.isfinite(res_0['total'])
            assert torch.allclose(res_d['total'][live], (res_0['total'] + seq_d)[live], rtol=1e-6, atol=2e-6)
            assert cases.BROUGHT_BACK_HYP not in _arr(res_d)[b0] and cases.BROUGHT_BACK_HYP not in _arr(res_0)[b0]
            # with the n-gram too, the first pass is the op with both
            lm = ngram_cases.golden_lm(3)[0]
            both = _rec(model, None, bias=pb, bias_first_pass=True, ngram_lm=lm, alpha=0.5, beta=1.0, **kw)
            res_b = both.rescore_pass(mem, mm, lp, ln)
            out = ops.ctc_prefix_beam_search_bias(lp, ln, pb, lm, 0.5, 1.0, beam_width=W, cutoff_top_n=K)
            for a, b in zip(res_b['beam'], out[:3]):
                assert torch.equal(a, b)
            assert torch.equal(res_b['ctc'], out[2] - out[3] - out[4])
            assert torch.equal(res_b['ng'], ops.ngram_score_sequences(lm, out[0], out[1], 0.5, 1.0, eos=cases.EOS))
    finally:
        ops.set_compute_dtype('bf16')
