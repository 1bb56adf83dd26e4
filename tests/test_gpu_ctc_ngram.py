"""GPU (-m gpu): the n-gram LM on the device.  otr_ngram_lookup against the dict-based restatement (tests/ngram_ref.py) and the
LM-fused CTC prefix beam search (otr_ctc_beam_search_lm, ops.ctc_prefix_beam_search_lm, CTCRecognizer ngram_lm=...) against
tests/ctc_prefix_lm_ref.py, brute force and the plain search.  tests/test_ngram.py asserts, without a GPU, that every input
compared here leaves at least the `min_clear` utterances clear of a near-tie."""
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import ops
from opentransformer_amd.ngram import NGramLM, min_capacity
from tests import ngram_cases as cases
from tests.ngram_ref import RefLM, make_lm
from tests.test_gpu_ctc_beam import hyps_of, load_c1
from tests.test_ngram import HAND_ARPA, HAND_UNITS, paths_by_string

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def lookup_queries(ref, rng, n):
    """contexts and tokens that cover a full hit, backoff over one and several levels, contexts that are not stored, contexts
    shorter than order-1, the <s> context, OOV tokens and OOV ids in the context"""
    V, N1 = ref.V, ref.order - 1
    grams = list(ref.grams)
    known = [g[0] for g in grams if len(g) == 1]
    ctxs, toks = [], []
    for q in range(n):
        kind = q % 6
        g = grams[rng.integers(len(grams))]
        if kind == 0:                                              # a stored n-gram: a hit at its own length
            c, t = g[:-1], g[-1]
        elif kind == 1:                                            # a stored context, a known token: mostly backoff
            c, t = g[:N1], known[rng.integers(len(known))]
        elif kind == 2:                                            # random known ids: the context is mostly not stored
            c = tuple(known[rng.integers(len(known))] for _ in range(rng.integers(N1 + 1)))
            t = known[rng.integers(len(known))]
        elif kind == 3:                                            # <s> first, as the search's contexts have it
            c, t = ((V,) + g[:-1])[:N1] if g[0] != V else g[:-1], g[-1]
        elif kind == 4:                                            # any id at all: OOV in either place
            c = tuple(int(rng.integers(V + 1)) for _ in range(rng.integers(N1 + 1)))
            t = int(rng.integers(V))
        else:                                                      # a stored n-gram behind one more id: cut or backed off
            c, t = ((known[rng.integers(len(known))],) + g[:-1])[-N1:] if N1 else (), g[-1]
        ctxs.append(tuple(c)[-N1:] if N1 else ())
        toks.append(int(t))
    return ctxs, toks


@pytest.mark.parametrize('order', [1, 2, 3, 5])
@pytest.mark.parametrize('V', [50, 4233])
def test_lookup_kernel_matches_the_restatement(order, V):
    """the table at the smallest legal capacity (chains longer than one entry); V = 4233 puts ids above 255 and 4096 into
    every key position"""
    per_order = ((300, 500, 600, 600) if V == 50 else (5000, 5000, 4000, 4000))[:order - 1]
    lm, ref = cases.lm_pair(11, V, order, per_order, absent=tuple(range(9, V, 10)), unk_unit=2)
    assert lm.capacity == min_capacity(lm.stats['entries'])
    if order > 1:
        assert lm.max_probe > 1
        top = np.array([g for g in ref.grams if len(g) == order])
        assert V == 50 or ((top > 4096).any(0).all() and ((top > 255) & (top < 4096)).any(0).all())
    ctxs, toks = lookup_queries(ref, np.random.default_rng(order), 3000)
    got = lm.lookup(ctxs, toks, device=DEV).cpu().numpy()
    host = lm.lookup_host(ctxs, toks)
    kinds = {}
    for c, t, g, h in zip(ctxs, toks, got, host):
        want = ref.cond(c, t)
        assert abs(g - want) <= 1e-6 * abs(want) + 1e-6, (c, t, g, want)
        assert abs(h - want) <= 1e-6 * abs(want) + 1e-6, (c, t, h, want)
        kind = 'oov' if want == ref.oov_score else 'hit' if c + (t,) in ref.grams else 'backoff'
        kinds[kind] = kinds.get(kind, 0) + 1
    assert all(kinds.get(k, 0) >= 30 for k in (('oov', 'hit', 'backoff') if order > 1 else ('oov', 'hit'))), kinds


def test_lookup_kernel_on_the_hand_written_lm():
    import io
    from tests.ngram_ref import LN10
    lm = NGramLM.from_arpa(io.StringIO(HAND_ARPA), HAND_UNITS)
    S, E, A, B, Cc = 5, 1, 2, 3, 4
    q = [((S, A), B, -0.2), ((S, A), E, -0.75), ((S, A), A, -1.25), ((B, B), A, -0.8), ((S,), A, -0.4), ((S,), B, -1.4),
         ((), A, -0.7), ((A,), B, -0.6), ((A,), Cc, None), ((Cc, B), A, None), ((B, Cc), A, None), ((A, B), 0, None)]
    got = lm.lookup([c for c, _, _ in q], [t for _, t, _ in q], device=DEV).cpu().numpy()
    for (c, t, v), g in zip(q, got):
        want = -1000.0 if v is None else v * LN10
        assert abs(g - want) <= 1e-6 * abs(want) + 1e-6, (c, t, g, want)


def run_lm(lp, lengths, lm, W, K, alpha=cases.ALPHA, beta=cases.BETA):
    out = ops.ctc_prefix_beam_search_lm(torch.from_numpy(lp).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV), lm,
                                        alpha, beta, beam_width=W, cutoff_top_n=K)
    return tuple(t.cpu().numpy() for t in out)


def check_against_reference(got, want, W, min_clear):
    """tests/test_gpu_ctc_beam.py's comparison with lm_scores added: wherever the restatement's W/W+1 gap exceeds 1e-4 at every
    frame the beams hold the same prefixes, scores and lm_scores within 1e-5 relative"""
    tokens, out_len, scores, lm_scores = got
    rt, rl, rs, rlm, gaps = want
    B, _, T = rt.shape
    assert tokens.shape == (B, W, T) and out_len.shape == (B, W) and scores.shape == (B, W) and lm_scores.shape == (B, W)
    clear = 0
    for b in range(B):
        s = scores[b]
        live = s > -math.inf
        assert (np.diff(s[live]) <= 0).all(), b
        assert not live[live.sum():].any()
        assert (out_len[b][~live] == 0).all() and (tokens[b][~live] == -1).all() and (lm_scores[b][~live] == 0).all()
        for r in range(W):
            assert (tokens[b, r, out_len[b, r]:] == -1).all() and (tokens[b, r, :out_len[b, r]] >= 0).all()
        if gaps[b] <= cases.GAP:
            continue
        clear += 1
        g_s, w_s = hyps_of(tokens, out_len, scores, b), hyps_of(rt, rl, rs, b)
        g_l = {tuple(tokens[b, r, :out_len[b, r]].tolist()): float(lm_scores[b, r]) for r in range(W) if live[r]}
        w_l = {tuple(rt[b, r, :rl[b, r]].tolist()): float(rlm[b, r]) for r in range(W) if rs[b, r] > -math.inf}
        assert set(g_s) == set(w_s), (b, W)
        for h, v in w_s.items():
            assert abs(g_s[h] - v) <= 1e-5 * abs(v) + 1e-6, (b, h, g_s[h], v)
            assert abs(g_l[h] - w_l[h]) <= 1e-5 * abs(w_l[h]) + 1e-6, (b, h, g_l[h], w_l[h])
        order_ok = all(abs(rs[b, r] - rs[b, r + 1]) <= cases.GAP or tuple(tokens[b, r, :out_len[b, r]]) == tuple(rt[b, r, :rl[b, r]])
                       for r in range(int(live.sum()) - 1))
        assert order_ok, b
    assert clear >= min_clear, (clear, gaps)


@pytest.mark.parametrize('order', cases.GOLDEN_ORDERS)
@pytest.mark.parametrize('K', cases.GOLDEN_KS)
@pytest.mark.parametrize('W', cases.GOLDEN_WS)
def test_search_matches_restatement_on_reference_log_probs(W, K, order):
    """the CTC head's log-probs of tests/golden/c1_decode.npz, full and ragged lengths, alpha 0.5, beta 1.0"""
    lp = cases.golden_log_probs()
    lm = cases.golden_lm(order)[0]
    for which, lengths in enumerate(cases.GOLDEN_LENGTHS):
        check_against_reference(run_lm(lp, lengths, lm, W, K), cases.golden_reference(W, K, order, which), W, min_clear=3)


def peaky(seed, B, T, V):
    rng = np.random.default_rng(seed)
    return torch.log_softmax(torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * 4.0), -1).numpy()


def test_zero_weights_give_the_plain_search_bit_for_bit():
    lp = torch.from_numpy(peaky(4, 5, 120, 4233)).to(DEV)
    ln = torch.tensor([120, 77, 1, 0, 119], dtype=torch.int32, device=DEV)
    lm = cases.size_lm()[0]
    plain = ops.ctc_prefix_beam_search(lp, ln, beam_width=10, cutoff_top_n=40)
    fused = ops.ctc_prefix_beam_search_lm(lp, ln, lm, 0.0, 0.0, beam_width=10, cutoff_top_n=40)
    for a, b in zip(plain, fused[:3]):
        assert torch.equal(a, b)
    assert (fused[3] == 0).all()
    b = 0.75                                               # alpha = 0: the addend is beta per token, exactly (0.75 * n in f32)
    tokens, out_len, scores, lm_scores = ops.ctc_prefix_beam_search_lm(lp, ln, lm, 0.0, b, beam_width=10, cutoff_top_n=40)
    assert torch.equal(lm_scores, b * out_len.float())
    assert int(out_len.max()) > 20


def test_the_lm_decides():
    """two frames in which unit a beats unit b acoustically by 0.1 nat; ln P(b | <s>) - ln P(a | <s>) = 2: the 1-best is [a] at
    alpha 0 and [b] at alpha 0.5"""
    import io
    ln10 = math.log(10.0)
    arpa = ('\\data\\\nngram 1=3\nngram 2=2\n\n\\1-grams:\n-99\t<s>\t0\n-1\tu2\t0\n-1\tu3\t0\n\n'
            '\\2-grams:\n%r\t<s> u2\n%r\t<s> u3\n\n\\end\\\n' % (-3.0 / ln10, -1.0 / ln10))
    lm = NGramLM.from_arpa(io.StringIO(arpa), {i: 'u%d' % i for i in range(5)})
    assert abs((lm.lookup_host([(5,)], [3]) - lm.lookup_host([(5,)], [2]))[0] - 2.0) < 1e-5
    p = np.full((1, 2, 5), 1e-6)                           # blank and the rest: next to nothing
    p[0, :, 2] = (1.0 - 3e-6) / (1.0 + math.exp(-0.05))    # a in both frames: collapses to [a]
    p[0, :, 3] = p[0, :, 2] * math.exp(-0.05)              # b: 0.05 nat less per frame
    lp = np.log(p).astype(np.float32)
    t0, l0, s0, _ = run_lm(lp, [2], lm, 4, 5, alpha=0.0, beta=0.0)
    t1, l1, s1, m1 = run_lm(lp, [2], lm, 4, 5, alpha=0.5, beta=0.0)
    acoustic = hyps_of(t0, l0, s0, 0)
    assert abs(acoustic[(2,)] - acoustic[(3,)] - 0.1) < 1e-3
    assert t0[0, 0, :l0[0, 0]].tolist() == [2]
    assert t1[0, 0, :l1[0, 0]].tolist() == [3]
    assert abs(m1[0, 0] - 0.5 * -1.0) < 1e-5


def test_exhaustive_on_the_device():
    """V = 3, T = 6, W = 32, K = 3, order 3: up to frame 5 the beam holds every string the frames can spell with two units (25
    of them), so nothing is pruned before the last selection (41 candidates at T = 6) and every live hypothesis carries the
    brute-force fused score; `a, blank, a` and its kin run the 1b merge with an addend"""
    rng = np.random.default_rng(13)
    V, T = 3, 6
    lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(4, T, V)) * 1.5), -1).numpy().astype(np.float32)
    lengths = [6, 6, 5, 4]
    import io
    text, grams, idx2unit = make_lm(2, V, 3, (4, 6))
    lm, ref = NGramLM.from_arpa(io.StringIO(text), idx2unit), RefLM(grams, 3, V)
    alpha, beta = 0.6, 0.3
    tokens, out_len, scores, lm_scores = run_lm(lp, lengths, lm, 32, 3, alpha, beta)
    for b, n in enumerate(lengths):
        every = paths_by_string(lp[b, :n].astype(np.float64))
        fused = {s: v + alpha * ref.score(s) + beta * len(s) for s, v in every.items()}
        best = sorted(fused, key=fused.get, reverse=True)
        got = hyps_of(tokens, out_len, scores, b)
        assert len(got) == min(32, len(every))
        assert tuple(tokens[b, 0, :out_len[b, 0]]) == best[0]
        if len(best) > 32 and fused[best[31]] - fused[best[32]] > cases.GAP:
            assert set(got) == set(best[:32])
        merged = 0
        for r in range(32):
            if scores[b, r] == -math.inf:
                continue
            s = tuple(tokens[b, r, :out_len[b, r]].tolist())
            want_lm = alpha * ref.score(s) + beta * len(s)
            assert abs(lm_scores[b, r] - want_lm) <= 1e-5 * abs(want_lm) + 1e-6, (b, s)
            assert abs(scores[b, r] - fused[s]) <= 1e-5 * abs(fused[s]) + 1e-6, (b, s, scores[b, r], fused[s])
            merged += any(s[j] == s[j + 1] for j in range(len(s) - 1))
        assert merged > 0 or n < 3


def test_at_size_against_the_restatement():
    """B = 6, T = 300, V = 4233, W 10, K 40, an order-3 LM of about 20 k n-grams that leaves units out"""
    lm = cases.size_lm()[0]
    got = run_lm(cases.size_log_probs(), cases.SIZE_LENGTHS, lm, 10, 40)
    check_against_reference(got, cases.size_reference(), 10, min_clear=5)
    tokens, out_len, scores, lm_scores = got
    assert out_len[0, 0] == 0 and scores[0, 0] == 0.0 and lm_scores[0, 0] == 0.0 and (tokens[0] == -1).all()
    assert np.isinf(scores[0, 1:]).all()


def test_recognizer_with_an_ngram_lm(golden):
    """CTCRecognizer(mode='beam', ngram_lm=lm): recognize is translate of the fused op's 1-best on the log-probs the assistor
    produced in the same call; recognize_with_times returns spans whose units spell the text"""
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
        lm = cases.golden_lm(3)[0]
        idx2unit = {i: str(i) for i in range(100)}
        rec = CTCRecognizer(model, idx2unit=idx2unit, mode='beam', beam_width=5, ngram_lm=lm, alpha=0.5, beta=1.0)
        texts = rec.recognize(x, m)
        lp, ln = seen[0]
        tokens, out_len, _, lm_scores = ops.ctc_prefix_beam_search_lm(lp, ln, lm, 0.5, 1.0, beam_width=5, cutoff_top_n=40)
        best = [tokens[b, 0, :int(out_len[b, 0])].tolist() for b in range(4)]
        assert texts == rec.translate(best)
        plain = ops.ctc_prefix_beam_search(lp, ln, beam_width=5, cutoff_top_n=40)
        assert not torch.equal(plain[2], ops.ctc_prefix_beam_search_lm(lp, ln, lm, 0.5, 1.0, beam_width=5)[2])
        assert float(lm_scores[:, 0].abs().sum()) > 0
        texts2, spans = rec.recognize_with_times(x, m)
        assert texts2 == texts
        for text, items in zip(texts, spans):
            assert ' '.join(u for u, _, _, _ in items) == text or [u for u, _, _, _ in items] == text.split()
            assert all(0 <= a < b <= 35 for _, a, b, _ in items)
    finally:
        ops.set_compute_dtype('bf16')
