"""GPU (-m gpu): n-gram LM fusion of the attention, joint and two-pass decoders (SpeechToTextRecognizer ngram_lm=...;
csrc/ngramattn.hip, otr_rescore_select_add) against the plain-Python restatement (tests/ngram_attn_ref.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from opentransformer_amd.ngram import NGramLM
from tests import ngram_attn_cases as cs
from tests import ngram_attn_ref as ref
from tests import rescore_ref
from tests.ngram_cases import lm_pair, size_lm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EOS = 1
NEG = -math.inf
ALPHA, BETA = 0.5, 1.0


class Memo:
    """a RefLM whose lookups are remembered: the cases of one LM share their (context, token) pairs"""

    def __init__(self, lm):
        self.lm, self.context, self.seen = lm, lm.context, {}

    def cond(self, ctx, c):
        key = (tuple(ctx), c)
        if key not in self.seen:
            self.seen[key] = self.lm.cond(ctx, c)
        return self.seen[key]


def close(got, want):
    """the lookup's bound of DESIGN.md 5.14: 1e-6 |v| + 1e-6"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-6


@functools.lru_cache(maxsize=None)
def cand_lm(name):
    if name == 'big':
        return size_lm() + (4233, tuple(range(50, 4233, 50)))                   # order 3, every 50th unit left out
    order = int(name)
    return lm_pair(40 + order, 50, order, (300, 400, 300, 200)[:order - 1], absent=(7, 13)) + (50, (7, 13))


def cand_inputs(rng, lm, V, absent, t, rows, K):
    """prefix rows of t columns (column 0 = BOS = the EOS id; an absent unit in some contexts), K distinct candidates per row -- an EOS
    candidate, two OOV candidates that get one score (equal totals: their addend is the same constant), a -inf score, a finished row --
    and scores chosen so that the totals sit on a grid of 0.25 between -20 and -40: no near-tie, and |total| of the addend's size."""
    oov = [0, absent[0], absent[1]]
    free = np.array([v for v in range(2, V) if v not in oov])
    preds = np.full((rows, t + 2), EOS, np.int64)
    preds[:, 1:t] = rng.choice(free, size=(rows, t - 1))
    idx = np.zeros((rows, K), np.int32)
    flags = np.zeros(rows, np.uint8)
    for r in range(rows):
        if t > 1 and r % 4 == 2:
            preds[r, rng.integers(1, t)] = absent[r % 2]                        # OOV inside the context
        idx[r] = rng.choice(free, size=K, replace=False)
        if r % 3 == 0:
            idx[r, 0] = EOS
        if K >= 4 and r % 2 == 0:
            idx[r, 1:3] = [oov[2], oov[1]]                                      # the higher token first
        flags[r] = rows > 1 and r % 4 == 1
    add = np.array(ref.score_candidates(lm, preds.tolist(), t, idx.tolist(), np.zeros((rows, K)).tolist(), ALPHA, BETA, EOS)[1])
    target = np.stack([-20.0 - 0.25 * rng.permutation(80)[:K] for _ in range(rows)])
    if K >= 4:
        target[::2, 2] = target[::2, 1]                                         # the OOV pair: one total
    score = (target - add).astype(np.float32)
    if K >= 4:
        score[::2, 2] = score[::2, 1]
    score[(np.arange(rows) % 5 == 3), K - 1] = NEG
    return preds, idx, score, flags


CAND_SHAPES = [(1, 1, (0, 1)), (1, 7, (5,)), (1, 32, (0, 16)), (5, 1, (1,)), (5, 7, (0, 1, 5)), (5, 32, (16,)), (65, 1, (0,)),
               (65, 7, (1, 5)), (65, 32, (0, 1, 5, 16))]


@pytest.mark.parametrize('name', ['1', '2', '3', '5', 'big'])
def test_candidate_kernel_matches_restatement(name):
    from opentransformer_amd import ops
    dev_lm, ref_lm, V, absent = cand_lm(name)
    lm = Memo(ref_lm)
    N = dev_lm.order
    rng = np.random.default_rng(7 * N + V)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    n_cases = n_oov = n_ties = 0
    for t in sorted({1, 2, max(N - 1, 1), N, N + 3}):
        for rows, K, beams in CAND_SHAPES:
            preds, idx, score, flags = cand_inputs(rng, lm, V, absent, t, rows, K)
            p_d, i_d, s_d, f_d = dev(preds), dev(idx), dev(score), dev(flags)
            pos = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
            for beam in beams:
                w_out, w_add, w_ks, w_ki = ref.score_candidates(lm, preds.tolist(), t, idx.tolist(), score.tolist(), ALPHA, BETA, EOS,
                                                                flags=flags.tolist(), beam=beam)
                out, add, ks, ki = ops.ngram_score_candidates(dev_lm, p_d, i_d, s_d, ALPHA, BETA, EOS, t=t, flags=f_d, beam=beam,
                                                              with_add=True)
                torch.cuda.synchronize()
                tag = (name, t, rows, K, beam)
                assert close(add.cpu().numpy(), w_add).all(), tag
                w_out = np.array(w_out)
                assert np.array_equal(np.isneginf(out.cpu().numpy()), np.isneginf(w_out)) and not torch.isnan(out).any(), tag
                fin = ~np.isneginf(w_out)
                assert close(out.cpu().numpy()[fin], w_out[fin]).all(), tag
                assert torch.equal(out[f_d.bool()], s_d[f_d.bool()]), tag                       # finished rows: copied
                if beam:
                    # the restatement's own gaps: nothing but the planted exact ties is closer than 1e-3
                    for r in range(rows):
                        if not flags[r]:
                            v = sorted(x for x in w_out[r] if x > NEG)
                            d = np.diff(v)
                            assert np.all((d == 0) | (d > 1e-3)), tag
                            n_ties += int((d == 0).sum())
                    assert ki.cpu().tolist() == w_ki, tag
                    w_ks = np.array(w_ks)
                    assert np.array_equal(np.isneginf(ks.cpu().numpy()), np.isneginf(w_ks)), tag
                    fin = ~np.isneginf(w_ks)
                    assert close(ks.cpu().numpy()[fin], w_ks[fin]).all(), tag
                # the device scalar pos and the host t: identical bits
                out2, add2, ks2, ki2 = ops.ngram_score_candidates(dev_lm, p_d, i_d, s_d, ALPHA, BETA, EOS, pos=pos, flags=f_d, beam=beam,
                                                                  with_add=True)
                assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(add2, add), tag
                assert beam == 0 or (torch.equal(ks2.view(torch.int32), ks.view(torch.int32)) and torch.equal(ki2, ki)), tag
                # alpha = beta = 0: cand_score, bit for bit
                out0 = ops.ngram_score_candidates(dev_lm, p_d, i_d, s_d, 0.0, 0.0, EOS, t=t, flags=f_d)[0]
                assert torch.equal(out0.view(torch.int32), s_d.view(torch.int32)), tag
                # in place
                s_in = s_d.clone()
                out3, _, ks3, ki3 = ops.ngram_score_candidates(dev_lm, p_d, i_d, s_in, ALPHA, BETA, EOS, t=t, flags=f_d, beam=beam,
                                                               cand_out=s_in)
                assert out3 is s_in and torch.equal(s_in.view(torch.int32), out.view(torch.int32)), tag
                assert beam == 0 or (torch.equal(ks3.view(torch.int32), ks.view(torch.int32)) and torch.equal(ki3, ki)), tag
                n_cases += 1
                n_oov += int((np.abs(np.array(w_add)) > 400).sum())
    assert n_cases >= 3 * 17 and n_oov > 50 and n_ties > 10


@pytest.mark.parametrize('order', [1, 2, 3, 5])
@pytest.mark.parametrize('n_hyp', [1, 33])
def test_sequence_kernel_matches_restatement(order, n_hyp):
    """lengths 0, 1, N-1 and 40 in turn, the padding behind a length ignored, a slot without a hypothesis (length -1) gives 0; the same
    bits on a second run.  Bound: each of the n + 1 lookups within 1e-6 |v| + 1e-6 (5.14), n f32 additions of at most 2^-24 of the sum
    of magnitudes each, and one rounding of alpha * sum + beta * n."""
    from opentransformer_amd import ops
    dev_lm, lm, V, absent = cand_lm(str(order))
    rng = np.random.default_rng(100 * order + n_hyp)
    T = 48
    lens = [(0, 1, max(order - 1, 0), 40)[(h + order) % 4] for h in range(n_hyp)]
    if n_hyp > 1:
        lens[5] = -1
    tok = np.full((n_hyp, T), -1, np.int64)
    for h, n in enumerate(lens):
        if n > 0:
            tok[h, :n] = rng.integers(1, V, size=n)                               # units 7 and 13 among them: OOV inside a sentence
    alpha, beta = 0.3, 0.8
    ln_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out, logp = ops.ngram_score_sequences(dev_lm, torch.from_numpy(tok).to(DEV), ln_d, alpha, beta, eos=EOS, with_logp=True)
    junk = tok.copy()
    junk[tok < 0] = -7
    for h, n in enumerate(lens):
        if n >= 0:
            junk[h, n:] = rng.integers(-5, V, size=T - n)                          # anything behind the length
    out2 = dev_lm.score(torch.from_numpy(junk).to(DEV), ln_d, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    n_big = 0
    for h, n in enumerate(lens):
        if n < 0:
            assert float(out[h]) == 0.0 and float(logp[h]) == 0.0
            continue
        seq = tok[h, :n].tolist()
        conds = [lm.cond(lm.context(seq[:j]), c) for j, c in enumerate(seq + [EOS])]
        want, want_lp = ref.seq_score(lm, seq, alpha, beta, EOS, with_logp=True)
        mag = sum(abs(c) for c in conds)
        tol_lp = 1e-6 * mag + 1e-6 * (n + 1) + n * 2.0 ** -24 * mag
        assert abs(float(logp[h]) - want_lp) <= tol_lp, (h, n, float(logp[h]), want_lp)
        assert abs(float(out[h]) - want) <= alpha * tol_lp + 2.0 ** -23 * (abs(alpha * want_lp) + beta * n), (h, n, float(out[h]), want)
        n_big += n == 40
    assert n_hyp == 1 or n_big >= 7
    empty = ops.ngram_score_sequences(dev_lm, torch.zeros((1, 0), dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                                      alpha, beta, eos=EOS)
    assert close(float(empty[0]), alpha * lm.cond(lm.context([]), EOS))


def _select(lib_fn, extra, tokens, out_len, ctc, n_rows, att, lm, nbest, lam, mu, penalty, lamda):
    from opentransformer_amd import _lib as L
    B, W, T = tokens.shape
    f32 = lambda *sh: torch.full(sh, 7.0, dtype=torch.float32, device=DEV)    # noqa: E731
    total, perm = f32(B, W), torch.zeros((B, W), dtype=torch.int32, device=DEV)
    nb_tok = torch.zeros((B, nbest, T), dtype=torch.int64, device=DEV)
    nb_len, nb_score = torch.zeros((B, nbest), dtype=torch.int32, device=DEV), f32(B, nbest)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None         # noqa: E731
    L.check(lib_fn(p(tokens), p(out_len), p(ctc), p(n_rows), p(att), p(lm), *extra, B, W, T, nbest, lam, mu, penalty, lamda, p(total), p(perm),
                   p(nb_tok), p(nb_len), p(nb_score), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'select')
    torch.cuda.synchronize()
    return total, perm, nb_tok, nb_len, nb_score


def test_rescore_select_add():
    """NULL add_score = otr_rescore_select bit for bit; an addend flips the 1-best; the penalty divides the sum that holds the addend"""
    from opentransformer_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(3)
    B, W, T, nbest = 3, 7, 9, 3
    out_len = torch.from_numpy(rng.integers(0, T + 1, size=(B, W)).astype(np.int32)).to(DEV)
    tokens = torch.from_numpy(rng.integers(2, 50, size=(B, W, T))).to(DEV)
    n_rows = out_len + 1
    n_rows[1, 4] = 0                                                              # a slot that is not rescorable
    f = lambda: torch.from_numpy(-rng.uniform(1.0, 30.0, size=(B, W)).astype(np.float32)).to(DEV)    # noqa: E731
    ctc, att, lm = f(), f(), f()
    lam, mu, pen, lamda = 0.3, 0.2, 0.6, 5.0
    args = (tokens, out_len, ctc, n_rows, att, lm, nbest, lam, mu, pen, lamda)
    base = _select(lib.otr_rescore_select, (), *args)
    null = _select(lib.otr_rescore_select_add, (None,), *args)
    for a, b in zip(base, null):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(a.view(torch.int32), b.view(torch.int32)))
    add = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    loser = int(base[1][0, W - 1])                                               # utterance 0's last-ranked slot
    add[0, loser] = 40.0
    add[2] = torch.from_numpy(rng.uniform(-3.0, 3.0, size=W).astype(np.float32)).to(DEV)
    got = _select(lib.otr_rescore_select_add, (C.c_void_p(add.data_ptr()),), *args)
    assert int(got[1][0, 0]) == loser != int(base[1][0, 0])
    assert torch.equal(got[2][0, 0], tokens[0, loser]) and int(got[3][0, 0]) == int(out_len[0, loser])
    a64, c64, l64, d64, n64 = (v.double().cpu().numpy() for v in (att, ctc, lm, add, out_len))
    for b in range(B):
        for w in range(W):
            if int(n_rows[b, w]) == 0:
                assert float(got[0][b, w]) == NEG
                continue
            inner = (1.0 - lam) * a64[b, w] + lam * c64[b, w] + mu * l64[b, w] + d64[b, w]
            want = inner / ((lamda + n64[b, w]) / (lamda + 1.0)) ** pen
            assert abs(float(got[0][b, w]) - want) <= 1e-6 * abs(want) + 1e-6, (b, w)
            outside = rescore_ref.total(a64[b, w], c64[b, w], l64[b, w], lam, mu, n64[b, w], pen, lamda) + d64[b, w]
            if abs(d64[b, w]) > 0.5 and n64[b, w] != 1:                           # (length 1: the penalty is 1)
                assert abs(float(got[0][b, w]) - outside) > 1e-3                   # the addend is inside the division
    order = [sorted(range(W), key=lambda i: (-float(got[0][b, i]), i)) for b in range(B)]
    assert got[1].cpu().tolist() == order


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


@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_search_matches_restatement_fp32(mode):
    """fp32, both loops: the restatement's tokens, scores within rtol 1e-5 / atol 1e-4 (the joint search's bound); the restatement,
    run on this device's encoder memory, is clear of near-ties (the seeds of tests/ngram_attn_cases.py)"""
    from opentransformer_amd import ops
    try:
        cfg, model, lm, x, m = _setup('fp32')
        par = cs.MODES[mode]
        dev_ng, ref_ng = cs.ngram(par['lm_seed'])
        with torch.no_grad():
            mem, mm, _, _ = _rec(model, None).encode(x, m)
        sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
        lsd = {k: v.float().cpu() for k, v in lm.state_dict().items()}
        want_h, want_s, gaps = cs.restated(cfg, sd, lsd, mem.float().cpu(), mm.cpu(), mode, ref_ng, par['alpha'], par['beta'])
        print('restatement gaps: min %.3g over %d cuts' % (min(gaps), len(gaps)))
        assert min(gaps) > cs.GAP
        assert sum(len(h[0]) for h in want_h) >= 10                               # the hypotheses are not all empty
        for cache in (False, True):
            rec = _rec(model, lm, joint_ctc=mode == 'joint', apply_cache=cache, ngram_lm=dev_ng, alpha=par['alpha'], beta=par['beta'])
            nb, sc = rec.recognize(x, m)
            print(mode, cache, 'max |d score| %.3g' % float((sc - want_s).abs().max()))
            assert _tok(nb) == want_h, (mode, cache)
            np.testing.assert_allclose(sc.numpy(), want_s.numpy(), rtol=1e-5, atol=1e-4)
        # and the n-gram matters: without it the 1-bests differ
        nb0, _ = _rec(model, lm, joint_ctc=mode == 'joint', apply_cache=True).recognize(x, m)
        assert [u[0] for u in _tok(nb0)] != [u[0] for u in want_h]
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_cached_matches_reforward_16bit(mode, dtype):
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup(dtype)
        par = cs.MODES[mode]
        kw = dict(joint_ctc=mode == 'joint', ngram_lm=cs.ngram(par['lm_seed'])[0], alpha=par['alpha'], beta=par['beta'])
        h0, s0 = _rec(model, lm, apply_cache=False, **kw).recognize(x, m)
        h1, s1 = _rec(model, lm, apply_cache=True, **kw).recognize(x, m)
        print(mode, dtype, 'scores', s0[:, :2].tolist(), s1[:, :2].tolist())
        assert [u[0] for u in h0] == [u[0] for u in h1]
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_graph_replay_and_a_swapped_lm(mode):
    """one recognizer (one CachedBeamState, replayed graphs) over two batches of one shape = fresh eager recognizers; another NGramLM
    put in its place builds a new state instead of replaying the old graph"""
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup('fp32')
        _, _, _, x2, m2 = _setup('fp32', seed=12)
        par = cs.MODES[mode]
        ng_a, ng_b = cs.ngram(par['lm_seed'])[0], cs.ngram(par['lm_seed'] + 2)[0]
        kw = dict(joint_ctc=mode == 'joint', apply_cache=True, alpha=par['alpha'], beta=par['beta'])
        shared = _rec(model, lm, ngram_lm=ng_a, **kw)
        got = [shared.recognize(x, m), shared.recognize(x2, m2), shared.recognize(x, m)]
        assert len(shared._cached_states) == 1
        shared.ngram_lm = ng_b
        got.append(shared.recognize(x, m))
        assert len(shared._cached_states) == 2
        for (xx, mm, ng), g in zip(((x, m, ng_a), (x2, m2, ng_a), (x, m, ng_a), (x, m, ng_b)), got):
            fresh = _rec(model, lm, ngram_lm=ng, **kw)
            fresh.use_hipgraph = False
            want = fresh.recognize(xx, mm)
            assert g[0] == want[0]
            np.testing.assert_allclose(g[1].numpy(), want[1].numpy(), rtol=1e-5, atol=1e-5)
        assert got[3][0] != got[0][0]                                             # the other LM decodes something else
    finally:
        ops.set_compute_dtype('bf16')


def test_rescore_with_ngram_fp32():
    """rescore=True: every slot's total is rescore_ref.total of the pass's own att / ctc / lm plus the restated n-gram score of the
    slot's string, inside the penalty; ctc is the first pass's score without its LM part; alpha = beta = 0 is the recognizer without
    an n-gram, bit for bit"""
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup('fp32')
        dev_ng, ref_ng = cs.ngram(5)
        alpha, beta, pen, lamda, max_len = 0.5, 1.0, 0.6, 5.0, 32     # max_len > T' + 1 = 30: every live slot is rescorable
        rec = _rec(model, lm, rescore=True, ngram_lm=dev_ng, alpha=alpha, beta=beta, penalty=pen, lamda=lamda, max_len=max_len)
        with torch.no_grad():
            mem, mm, _, _ = rec.encode(x, m)
            log_probs, length = model.assistor.inference(mem, mm)
            log_probs = log_probs.float().contiguous()
            res = rec.rescore_pass(mem, mm, log_probs, length)
            first = ops.ctc_prefix_beam_search_lm(log_probs, length, dev_ng, alpha, beta, beam_width=cs.BEAM, cutoff_top_n=40,
                                                  blank=model.assistor.blank)
        tokens, out_len, scores = (v.cpu() for v in res['beam'])
        assert torch.equal(tokens, first[0].cpu()) and torch.equal(scores, first[2].cpu())
        assert torch.equal(res['ctc'].cpu(), (first[2] - first[3]).cpu())
        checked = 0
        for b in range(tokens.shape[0]):
            for w in range(tokens.shape[1]):
                n = int(out_len[b, w])
                if not (float(scores[b, w]) > NEG and n + 1 <= max_len):
                    assert float(res['total'][b, w]) == NEG
                    continue
                h = tokens[b, w, :n].tolist()
                ng = ref.seq_score(ref_ng, h, alpha, beta, EOS)
                assert abs(float(res['ng'][b, w]) - ng) <= 1e-5 * abs(ng) + 1e-5
                inner = rescore_ref.total(float(res['att'][b, w]), float(res['ctc'][b, w]), float(res['lm'][b, w]), cs.LAMBDA, cs.LM_WEIGHT,
                                          n) + ng
                want = inner / ((lamda + n) / (lamda + 1.0)) ** pen
                assert abs(float(res['total'][b, w]) - want) <= 1e-5 * abs(want) + 1e-4, (b, w)
                checked += 1
        assert checked >= 12
        plain = _rec(model, lm, rescore=True, penalty=pen, lamda=lamda, max_len=max_len).recognize(x, m)
        zero = _rec(model, lm, rescore=True, ngram_lm=dev_ng, alpha=0.0, beta=0.0, penalty=pen, lamda=lamda, max_len=max_len).recognize(x, m)
        assert plain[0] == zero[0] and torch.equal(plain[1], zero[1])
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['plain', 'joint', 'rescore'])
def test_an_lm_against_the_acoustic_best_changes_it(mode):
    """an order-1 LM that gives the tokens of the acoustic 1-best of utterance 0 (</s> itself where that 1-best is empty, as the flat
    synthetic decoder's is in the plain search) a log-prob of -50 and every other unit -1"""
    from opentransformer_amd import ops
    try:
        _, model, lm, x, m = _setup('fp32')
        kw = dict(joint_ctc=mode == 'joint', rescore=mode == 'rescore', apply_cache=mode != 'rescore', max_len=24)
        base, _ = _rec(model, lm, **kw).recognize(x, m)
        best = _tok(base)[0][0]
        V = 100
        ids = np.arange(V + 1).reshape(-1, 1)
        logp = np.full(V + 1, -1.0, np.float32)
        logp[sorted(set(best)) or [EOS]] = -50.0
        against = NGramLM(1, V, ids, np.ones(V + 1, np.int64), logp, np.zeros(V + 1, np.float32))
        got, _ = _rec(model, lm, ngram_lm=against, alpha=1.0, beta=0.0, **kw).recognize(x, m)
        assert _tok(got)[0][0] != best
        assert not set(_tok(got)[0][0]) & set(best) and (best or _tok(got)[0][0])
    finally:
        ops.set_compute_dtype('bf16')


def test_limits_are_refused_before_any_launch():
    from opentransformer_amd import ops
    try:
        _, model, lm, _, _ = _setup('fp32', with_lm=False)
        ng = cs.ngram(5)[0]
        with pytest.raises(NotImplementedError, match='NGramLM'):
            _rec(model, None, ngram_lm='lm.arpa')
        with pytest.raises(ValueError, match='beam_width'):
            _rec(model, None, ngram_lm=ng, beam_width=17)
        for bad in (4, 33, 101):
            with pytest.raises(ValueError, match='ngram_beam'):
                _rec(model, None, ngram_lm=ng, ngram_beam=bad)
        with pytest.raises(ValueError, match='units'):
            _rec(model, None, ngram_lm=lm_pair(2, 50, 2, (300,))[0])
        assert _rec(model, None, ngram_lm=ng).ngram_beam == 7
    finally:
        ops.set_compute_dtype('bf16')
