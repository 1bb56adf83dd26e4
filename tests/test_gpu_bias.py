"""GPU (-m gpu): phrase biasing of the attention, joint and two-pass decoders (SpeechToTextRecognizer bias=...; csrc/bias.hip) against
the plain-Python restatement (tests/bias_ref.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from opentransformer_amd.bias import PhraseBias
from tests import bias_cases as cs
from tests import bias_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EOS = 1
NEG = -math.inf
F32 = np.float32
V = 50
LDP = 24
P16 = (10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25)


@functools.lru_cache(maxsize=None)
def kernel_set(dyadic=False):
    """V = 50: a 16-id phrase, a 1-id phrase, phrases that are prefixes / suffixes of others (3 4 5 6 fails over to 4 5 6 8's
    4 5 6), one that overlaps itself, and 20 random ones; f32 weights with full mantissas (or dyadic ones)"""
    rng = np.random.default_rng(21)
    phrases = [P16, (7,), (3, 4, 5), (4, 5, 6, 8), (3, 4), (9, 9, 9), (5, 6), P16[8:] + (30, 31)]
    units = [v for v in range(V) if v != EOS]
    phrases += [tuple(int(v) for v in rng.choice(units, size=rng.integers(2, 7))) for _ in range(20)]
    if dyadic:
        weights = [float(w) for w in rng.choice([0.25, 0.5, 1.0, 2.0], size=len(phrases))]
    else:
        weights = [float(F32(w)) for w in rng.uniform(0.1, 3.0, size=len(phrases))]
    return PhraseBias(phrases, V, weights=weights), ref.RefBias(phrases, weights, V, EOS), phrases


def tail_for(rng, phrases, r):
    """the newest tokens of prefix row r (right aligned at column t - 1): a phrase entered and not left, so that the state is deep"""
    kind = r % 6
    if kind == 0:
        return list(P16)                                        # the whole 16-id phrase: an end node of depth 16
    if kind == 1:
        return list(P16[:15])                                   # one short of it: the candidate P16[15] completes it
    if kind == 2:
        return [3, 4, 5, 6]                                     # no node: the match fails over to 4 5 6 (of 4 5 6 8)
    if kind == 3:
        return [9, 9, 9, 9]                                     # past the end of 9 9 9: the suffix 9 9 9 again
    q = phrases[int(rng.integers(0, len(phrases)))]
    if kind == 4:
        return list(q[:int(rng.integers(1, len(q) + 1))])
    return list(P16[:8]) + list(P16[8:])[:int(rng.integers(1, 8))]


def cand_inputs(rng, rb, phrases, t, rows, K):
    """prefix rows of t columns (column 0 = BOS = the EOS id) in LDP-wide rows, K distinct candidates per row -- the tokens that go
    on from the state, EOS, two tokens no phrase starts with that get one score (equal totals: the higher token first) -- a -inf and
    a NaN score, ids >= V and < 0 in some prefixes, finished rows"""
    free = np.array([v for v in range(2, V) if not any(p[0] == v for p in phrases)])
    preds = np.full((rows, LDP), EOS, np.int64)
    idx = np.zeros((rows, K), np.int32)
    score = (-20.0 - 0.25 * np.stack([rng.permutation(80)[:K] for _ in range(rows)])).astype(np.float32)
    flags = np.zeros(rows, np.uint8)
    for r in range(rows):
        preds[r, 1:t] = rng.choice(np.arange(2, V), size=t - 1)
        tail = tail_for(rng, phrases, r)[-(t - 1):] if t > 1 else []
        if tail:
            preds[r, t - len(tail):t] = tail
        if t > 2 and r % 7 == 5:
            preds[r, int(rng.integers(1, t))] = (V, -1, V + 7, -(2 ** 40))[r % 4]     # a token in no phrase, maybe inside the match
        preds[r, t:] = rng.integers(-3, V + 3, size=LDP - t)      # whatever lies behind the prefix is not read
        st = rb.state(preds[r, 1:t].tolist())
        go_on = sorted({p[len(st)] for p in phrases if len(p) > len(st) and p[:len(st)] == st})
        pool = [EOS, int(free[-1]), int(free[0])] + go_on + [7]
        rest = [int(v) for v in rng.permutation(np.arange(2, V)) if v not in pool]
        pick = pool if r % 2 == 0 else go_on + [EOS]              # (K = 1: EOS behind the match, or the token that goes on)
        idx[r] = list(dict.fromkeys(pick + rest))[:K]
        if K >= 5 and r % 2 == 0:
            a, b = list(idx[r]).index(int(free[-1])), list(idx[r]).index(int(free[0]))
            score[r, b] = score[r, a]                             # both lead to the root: one addend, one total
        if K > 1 and r % 5 == 3:
            score[r, K - 1] = NEG
        if K > 2 and r % 5 == 1:
            score[r, K - 2] = np.nan
        flags[r] = rows > 1 and r % 4 == 1
    return preds, idx, score, flags


def same_bits(got, want):
    """f32 arrays: the same bits, NaN matching NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize('K', [1, 5, 32])
def test_candidate_kernel_matches_restatement(K):
    """rows at the workgroup's edge (8 rows each), t around the phrase depth (16) and at ldp, the host t and the device pos, with and
    without flags, no select / top-1 / top-min(16, K): cand_out, cand_add, k_score and k_idx bit for bit; in place; nothing written
    behind the rows"""
    from opentransformer_amd import ops
    pb, rb, phrases = kernel_set()
    rng = np.random.default_rng(100 + K)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    pb.to(DEV)
    seen = dict(cases=0, pos=0, neg=0, ties=0, deep=0, nan=0)
    for rows in (1, 7, 8, 9, 17):
        for t in (1, 2, 16, 17, 18, LDP):
            preds, idx, score, flags = cand_inputs(rng, rb, phrases, t, rows, K)
            p_d, i_d, s_d, f_d = dev(preds), dev(idx), dev(score), dev(flags)
            pos = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
            for fl, fl_d in ((None, None), (flags.tolist(), f_d)):
                for beam in sorted({0, 1, min(16, K)}):
                    w_out, w_add, w_ks, w_ki = ref.score_candidates(rb, preds.tolist(), t, idx.tolist(), score.tolist(), EOS, flags=fl,
                                                                    beam=beam)
                    tag = (K, rows, t, fl is not None, beam)
                    for kw in (dict(t=t), dict(pos=pos)):
                        out_full = torch.full((rows + 1, K), 7.0, dtype=torch.float32, device=DEV)
                        ks_full = torch.full((rows + 1, max(beam, 1)), 7.0, dtype=torch.float32, device=DEV)
                        ki_full = torch.full((rows + 1, max(beam, 1)), 7, dtype=torch.int64, device=DEV)
                        out, add, ks, ki = ops.bias_score_candidates(pb, p_d, i_d, s_d, EOS, flags=fl_d, beam=beam, with_add=True,
                                                                     cand_out=out_full[:rows], k_score=ks_full[:rows] if beam else None,
                                                                     k_idx=ki_full[:rows] if beam else None, **kw)
                        torch.cuda.synchronize()
                        assert float(out_full[rows].min()) == 7.0 == float(out_full[rows].max()), tag
                        assert float(ks_full[rows].min()) == 7.0 and int(ki_full[rows].min()) == 7, tag
                        assert same_bits(out.cpu().numpy(), w_out), tag
                        assert same_bits(add.cpu().numpy(), w_add), tag
                        if beam:
                            assert ki.cpu().tolist() == w_ki, tag
                            assert same_bits(ks.cpu().numpy(), w_ks), tag
                    s_in = s_d.clone()                                             # in place
                    out3, _, ks3, ki3 = ops.bias_score_candidates(pb, p_d, i_d, s_in, EOS, t=t, flags=fl_d, beam=beam, cand_out=s_in)
                    assert out3 is s_in and same_bits(s_in.cpu().numpy(), w_out), tag
                    assert beam == 0 or (ki3.cpu().tolist() == w_ki and same_bits(ks3.cpu().numpy(), w_ks)), tag
                    seen['cases'] += 1
            a = np.array(w_add)
            live = flags == 0
            seen['pos'] += int((a[live] > 0).sum())
            seen['neg'] += int((a[live] < 0).sum())
            seen['nan'] += int(np.isnan(score[live]).sum())
            seen['deep'] += sum(len(rb.state(preds[r, 1:t].tolist())) >= 15 for r in range(rows))
            for r in np.flatnonzero(live):
                v = np.array(w_out[r])
                v = v[np.isfinite(v)]
                seen['ties'] += len(v) - len(np.unique(v))
    print(K, seen)
    assert seen['cases'] == 5 * 6 * 2 * len({0, 1, min(16, K)})
    assert seen['pos'] > 10 and seen['neg'] > 10 and seen['deep'] > 5
    assert K < 5 or (seen['ties'] > 5 and seen['nan'] > 5)


def seq_inputs(rng, phrases, n_hyp, T):
    """hypotheses of length 0, 1 and T in turn (and some in between) made of phrases, pieces of phrases and other tokens; a slot
    without a hypothesis (length -1); anything behind a length"""
    lens = [(0, 1, T, T, max(T // 2, 1))[h % 5] for h in range(n_hyp)]
    if n_hyp > 1:
        lens[min(5, n_hyp - 1)] = -1
    tok = rng.integers(-5, V + 5, size=(n_hyp, T)).astype(np.int64)
    for h, n in enumerate(lens):
        x = []
        while len(x) < max(n, 0):
            kind = rng.integers(0, 4)
            q = phrases[int(rng.integers(0, len(phrases)))] if h % 3 else P16
            if kind == 0:
                x += [int(v) for v in rng.integers(-2, V + 2, size=rng.integers(1, 3))]
            elif kind == 1:
                x += q[:int(rng.integers(1, len(q) + 1))]
            else:
                x += q
        tok[h, :max(n, 0)] = x[:max(n, 0)]
    return tok, lens


@pytest.mark.parametrize('T', [1, 16, 17, 40, 130])
@pytest.mark.parametrize('n_hyp', [1, 63, 64, 65])
def test_sequence_kernel_matches_restatement(n_hyp, T):
    """dyadic weights: the restatement's value exactly; f32 weights: within (L + 1) * 2^-24 * sum |addends|, L + 1 additions of at
    most half an ulp of a partial sum each.  T = 130 is past one wave of positions (the chunk loop and its carry).  A second run
    gives the same bits; a slot without a hypothesis gives 0."""
    from opentransformer_amd import ops
    rng = np.random.default_rng(1000 * T + n_hyp)
    tok, lens = seq_inputs(rng, kernel_set()[2], n_hyp, T)
    tok_d = torch.from_numpy(tok).to(DEV)
    ln_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    completed = 0
    for dyadic in (True, False):
        pb, rb, _ = kernel_set(dyadic)
        out = ops.bias_score_sequences(pb, tok_d, ln_d, eos=EOS)
        out2 = pb.score(tok_d.view(1, n_hyp, T), ln_d.view(1, n_hyp))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32).view(-1))
        got = out.cpu().numpy()
        for h, n in enumerate(lens):
            if n < 0:
                assert got[h] == 0.0
                continue
            adds = ref.addends(rb, tok[h, :n].tolist(), EOS)
            want = ref.seq_score(rb, tok[h, :n].tolist(), EOS)
            if dyadic:
                assert got[h] == want == sum(float(a) for a in adds) >= 0.0, (h, n, got[h], want)
            else:
                exact = sum(float(a) for a in adds)
                assert abs(float(got[h]) - exact) <= (n + 1) * 2.0 ** -24 * sum(abs(float(a)) for a in adds), (h, n, got[h], exact)
            completed += got[h] > 0.2
    assert n_hyp == 1 or T == 1 or completed >= 10
    with pytest.raises(Exception, match='CUDA/HIP'):
        ops.bias_score_sequences(pb, tok_d.cpu(), ln_d.cpu())


# ---------------------------------------------------------------- the recognizer
def _setup(mode, with_lm=True, seed=cs.INPUT_SEED):
    import opentransformer_amd as ota
    from opentransformer_amd import ops, synthetic as syn
    from opentransformer_amd.recognize import LanguageModel
    ops.set_compute_dtype(mode)
    cfg = cs.model_cfg()
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).eval()
    lm = None
    if with_lm:
        lm = LanguageModel['transformer_lm'](cs.LM_CFG)
        syn.fill_state_dict_(lm.state_dict(), 4321)
        lm = lm.to(DEV).eval()
    x, m = cs.batch(seed)
    return cfg, model, lm, x.to(DEV), m.to(DEV)


def _rec(model, lm, **kw):
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    kw.setdefault('beam_width', cs.BEAM)
    kw.setdefault('nbest', cs.NBEST)
    kw.setdefault('max_len', cs.MAX_LEN)
    return SpeechToTextRecognizer(model, lm=lm, idx2unit={i: str(i) for i in range(100)}, ngpu=1, lm_weight=cs.LM_WEIGHT,
                                  ctc_weight=cs.LAMBDA, **kw)


def _tok(nbest):
    return [[[int(t) for t in s.split()] for s in utt] for utt in nbest]


def _ngram_kw(mode, with_ngram):
    """(recognizer keywords, the RefLM or None, alpha, beta) of a case"""
    if not with_ngram:
        return {}, None, 0.0, 0.0
    par = cs.MODES[mode]
    dev_ng, ref_ng = cs.ngram(par['lm_seed'])
    return dict(ngram_lm=dev_ng, alpha=par['alpha'], beta=par['beta']), ref_ng, par['alpha'], par['beta']


@pytest.mark.parametrize('with_ngram', [False, True])
@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_search_matches_restatement_fp32(mode, with_ngram):
    """fp32, both loops, with and without the n-gram of tests/ngram_attn_cases.py: the restatement's tokens, scores within rtol 1e-5 /
    atol 1e-4 (test_gpu_ngram_attn.py::test_search_matches_restatement_fp32's bound: the same arithmetic plus one f32 addition per
    step); the restatement, run on this device's encoder memory, is clear of near-ties; and the phrases change the 1-best"""
    from opentransformer_amd import ops
    try:
        cfg, model, lm, x, m = _setup('fp32')
        kw, ref_ng, alpha, beta = _ngram_kw(mode, with_ngram)
        pb, rb = cs.phrase_set(mode, with_ngram)
        with torch.no_grad():
            mem, mm, _, _ = _rec(model, None).encode(x, m)
        sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
        lsd = {k: v.float().cpu() for k, v in lm.state_dict().items()}
        want_h, want_s, gaps = cs.restated(cfg, sd, lsd, mem.float().cpu(), mm.cpu(), mode, rb, ref_ng, alpha, beta)
        print('restatement gaps: min %.3g over %d cuts' % (min(gaps), len(gaps)))
        assert min(gaps) > cs.GAP
        for cache in (False, True):
            rec = _rec(model, lm, joint_ctc=mode == 'joint', apply_cache=cache, bias=pb, **kw)
            nb, sc = rec.recognize(x, m)
            print(mode, with_ngram, cache, 'max |d score| %.3g' % float((sc - want_s).abs().max()))
            assert _tok(nb) == want_h, (mode, cache)
            np.testing.assert_allclose(sc.numpy(), want_s.numpy(), rtol=1e-5, atol=1e-4)
        nb0, _ = _rec(model, lm, joint_ctc=mode == 'joint', apply_cache=True, **kw).recognize(x, m)
        assert [u[0] for u in _tok(nb0)] != [u[0] for u in want_h]
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_cached_matches_reforward_16bit(mode, dtype):
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup(dtype)
        kw = dict(_ngram_kw(mode, True)[0], joint_ctc=mode == 'joint', bias=cs.phrase_set(mode, True)[0])
        h0, s0 = _rec(model, lm, apply_cache=False, **kw).recognize(x, m)
        h1, s1 = _rec(model, lm, apply_cache=True, **kw).recognize(x, m)
        print(mode, dtype, 'scores', s0[:, :2].tolist(), s1[:, :2].tolist())
        assert [u[0] for u in h0] == [u[0] for u in h1]
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_graph_replay_and_a_swapped_phrase_set(mode):
    """one recognizer (one CachedBeamState, replayed graphs) over two batches of one shape = fresh eager recognizers; another
    PhraseBias put in its place builds a second state instead of replaying the old graph, and decodes something else"""
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup('fp32')
        _, _, _, x2, m2 = _setup('fp32', seed=12)
        pb_a, pb_b = cs.phrase_set(mode, False)[0], cs.phrase_set('joint' if mode == 'plain' else 'plain', False)[0]
        kw = dict(joint_ctc=mode == 'joint', apply_cache=True)
        shared = _rec(model, lm, bias=pb_a, **kw)
        got = [shared.recognize(x, m), shared.recognize(x2, m2), shared.recognize(x, m)]
        assert len(shared._cached_states) == 1
        shared.bias = pb_b
        got.append(shared.recognize(x, m))
        assert len(shared._cached_states) == 2
        for (xx, mm, pb), g in zip(((x, m, pb_a), (x2, m2, pb_a), (x, m, pb_a), (x, m, pb_b)), got):
            fresh = _rec(model, lm, bias=pb, **kw)
            fresh.use_hipgraph = False
            want = fresh.recognize(xx, mm)
            assert g[0] == want[0]
            np.testing.assert_allclose(g[1].numpy(), want[1].numpy(), rtol=1e-5, atol=1e-5)
        assert got[3][0] != got[0][0]
    finally:
        ops.set_compute_dtype('bf16')


def test_rescore_with_phrases_fp32():
    """rescore=True: the first pass is the unbiased one; res['bias'] is the restated phrase score of every first-pass hypothesis
    (dyadic weights: exactly); every total is the pass's own att / ctc / lm plus that term INSIDE the length division (the bound of
    test_gpu_ngram_attn.py::test_rescore_select_add: 1e-6 |v| + 1e-6); a phrase equal to a lower-ranked hypothesis, with enough
    weight, moves it to rank 0"""
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup('fp32')
        pen, lamda, max_len = 0.6, 5.0, 32                       # max_len > T' + 1 = 30: every live slot is rescorable
        kw = dict(rescore=True, penalty=pen, lamda=lamda, max_len=max_len)
        base = _rec(model, lm, **kw)
        with torch.no_grad():
            mem, mm, _, _ = base.encode(x, m)
            log_probs, length = model.assistor.inference(mem, mm)
            log_probs = log_probs.float().contiguous()
            res0 = base.rescore_pass(mem, mm, log_probs, length)
        assert res0['bias'] is None
        tokens, out_len, scores = (v.cpu() for v in res0['beam'])
        B, W, _ = tokens.shape
        hyps = [[tuple(tokens[b, w, :int(out_len[b, w])].tolist()) for w in range(W)] for b in range(B)]
        live = [[float(scores[b, w]) > NEG and int(out_len[b, w]) + 1 <= max_len for w in range(W)] for b in range(B)]
        pf = lambda n: ((lamda + n) / (lamda + 1.0)) ** pen       # noqa: E731
        # phrases cut from the hypotheses themselves: pieces of them complete inside other hypotheses too
        pieces = sorted({h[a:a + n] for row in hyps for h in row for n in (1, 2, 3) for a in range(0, max(len(h) - n + 1, 0), 2)})
        pieces = [p for p in pieces if EOS not in p][:40]
        assert len(pieces) >= 3
        weights = [(0.25, 0.5, 1.0)[i % 3] for i in range(len(pieces))]
        pb, rb = PhraseBias(pieces, cs.V, weights=weights), ref.RefBias(pieces, weights, cs.V, EOS)
        with torch.no_grad():
            res1 = _rec(model, lm, bias=pb, **kw).rescore_pass(mem, mm, log_probs, length)
        for a, b in zip(res0['beam'], res1['beam']):
            assert torch.equal(a, b)                             # the first pass is not biased
        checked = moved = 0
        for b in range(B):
            for w in range(W):
                if not live[b][w]:
                    assert float(res1['total'][b, w]) == NEG
                    continue
                n = len(hyps[b][w])
                term = float(ref.seq_score(rb, hyps[b][w], EOS))
                assert float(res1['bias'][b, w]) == term, (b, w)
                inner = (1.0 - cs.LAMBDA) * float(res1['att'][b, w]) + cs.LAMBDA * float(res1['ctc'][b, w]) \
                    + cs.LM_WEIGHT * float(res1['lm'][b, w]) + term
                want = inner / pf(n)
                assert abs(float(res1['total'][b, w]) - want) <= 1e-6 * abs(want) + 1e-6, (b, w)
                want0 = float(res0['total'][b, w]) + term / pf(n)             # the unbiased total plus the term inside the division
                assert abs(float(res1['total'][b, w]) - want0) <= 1e-6 * abs(want0) + 2e-6, (b, w)
                if term > 0.5 and n != 1:
                    assert abs(float(res1['total'][b, w]) - (float(res0['total'][b, w]) + term)) > 1e-3
                checked += 1
                moved += term > 0.0
        assert checked >= 12 and moved >= 6
        # a lower-ranked hypothesis as a phrase: the lowest-ranked live slot of an utterance whose string no other slot contains
        done = False
        for b in range(B):
            perm = res0['perm'][b].cpu().tolist()
            ranked = [w for w in perm if live[b][w]]
            for w in reversed(ranked[1:]):
                h = hyps[b][w]
                contains = lambda g: any(g[a:a + len(h)] == h for a in range(len(g) - len(h) + 1))      # noqa: E731
                if not 1 <= len(h) <= 16 or EOS in h or any(contains(hyps[b][o]) for o in ranked if o != w):
                    continue
                gap = (float(res0['total'][b, ranked[0]]) - float(res0['total'][b, w])) * pf(len(h)) * pf(max_len)
                wt = math.ceil(2.0 * gap / len(h) + 1.0)
                got, _ = _rec(model, lm, bias=PhraseBias([h], cs.V, weights=[wt]), **kw).recognize(x, m)
                before, _ = base.recognize(x, m)
                assert _tok(got)[b][0] == list(h) != _tok(before)[b][0], (b, w, h, wt)
                done = True
                break
            if done:
                break
        assert done
    finally:
        ops.set_compute_dtype('bf16')


def test_limits_are_refused_before_any_launch():
    from opentransformer_amd import _lib, ops
    try:
        _, model, lm, _, _ = _setup('fp32', with_lm=False)
        pb = cs.phrase_set('plain', False)[0]
        with pytest.raises(TypeError, match='PhraseBias'):
            _rec(model, None, bias=[[2, 3]])
        with pytest.raises(ValueError, match='beam_width'):
            _rec(model, None, bias=pb, beam_width=17)
        for bad in (4, 33, 101):
            with pytest.raises(ValueError, match='bias_beam'):
                _rec(model, None, bias=pb, bias_beam=bad)
        with pytest.raises(ValueError, match='units'):
            _rec(model, None, bias=PhraseBias([[2, 3]], 50))
        with pytest.raises(ValueError, match='ngram_beam'):
            _rec(model, None, bias=pb, bias_beam=9, ngram_lm=cs.ngram(5)[0], ngram_beam=8)
        assert _rec(model, None, bias=pb).bias_beam == 7
        p = torch.zeros((4, 8), dtype=torch.int64, device=DEV)
        for K, beam in ((33, 0), (8, 9), (20, 17)):
            ci, sc = torch.zeros((4, K), dtype=torch.int32, device=DEV), torch.zeros((4, K), dtype=torch.float32, device=DEV)
            with pytest.raises(_lib.OtransHipError, match='bias_score_cands'):
                ops.bias_score_candidates(pb, p, ci, sc, EOS, t=1, beam=beam)
        ci, sc = torch.zeros((4, 8), dtype=torch.int32, device=DEV), torch.zeros((4, 8), dtype=torch.float32, device=DEV)
        with pytest.raises(_lib.OtransHipError, match='bias_score_cands'):
            ops.bias_score_candidates(pb, p, ci, sc, EOS, t=9)
        with pytest.raises(_lib.OtransHipError, match='CUDA/HIP'):
            ops.bias_score_candidates(pb, p.cpu(), ci.cpu(), sc.cpu(), EOS, t=1)
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype('bf16')
