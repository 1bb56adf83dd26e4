"""GPU (-m gpu): CTC prefix beam search on the device (otr_ctc_topk + otr_ctc_beam_search, ops.ctc_prefix_beam_search,
CTCRecognizer mode='beam') against the plain-Python restatement tests/ctc_prefix_ref.py."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, ops
from opentransformer_amd import synthetic as syn
from tests import ctc_prefix_ref as ref
from tests.test_ctc_beam import ctc_logprob

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def hyps_of(tokens, out_len, scores, b):
    """utterance b's live hypotheses as {token tuple: score}"""
    return {tuple(tokens[b, r, :out_len[b, r]].tolist()): float(scores[b, r])
            for r in range(tokens.shape[1]) if scores[b, r] > -math.inf}


def check_against_reference(lp, lengths, W, K, gap=1e-4, min_clear=None):
    """run the device search and the restatement; wherever the restatement's W/W+1 boundary gap exceeds `gap` at every frame the
    two beams hold the same prefixes with scores within 1e-5 relative; returns the number of such utterances"""
    x = torch.from_numpy(lp).to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    tokens, out_len, scores = (t.cpu().numpy() for t in ops.ctc_prefix_beam_search(x, ln, beam_width=W, cutoff_top_n=K))
    gaps = []
    rt, rl, rs = ref.decode(lp, lengths, W, K, min_gap=gaps)
    B, T = lp.shape[:2]
    assert tokens.shape == (B, W, T) and out_len.shape == (B, W) and scores.shape == (B, W)
    clear = 0
    for b in range(B):
        s = scores[b]
        live = s > -math.inf
        assert (np.diff(s[live]) <= 0).all(), b                        # descending
        assert not live[live.sum():].any()                             # live slots first
        assert (out_len[b][~live] == 0).all() and (tokens[b][~live] == -1).all()
        for r in range(W):
            assert (tokens[b, r, out_len[b, r]:] == -1).all() and (tokens[b, r, :out_len[b, r]] >= 0).all()
        if gaps[b] <= gap:
            continue
        clear += 1
        got, want = hyps_of(tokens, out_len, scores, b), hyps_of(rt, rl, rs, b)
        assert set(got) == set(want), (b, W, K)
        for h, v in want.items():
            assert abs(got[h] - v) <= 1e-5 * abs(v) + 1e-6, (b, h, got[h], v)
        # the order too, wherever neighbours are apart
        order_ok = all(abs(rs[b, r] - rs[b, r + 1]) <= gap or tuple(tokens[b, r, :out_len[b, r]]) == tuple(rt[b, r, :rl[b, r]])
                       for r in range(int(live.sum()) - 1))
        assert order_ok, b
    if min_clear is not None:
        assert clear >= min_clear, (clear, gaps)
    return clear


@pytest.mark.parametrize('W', [1, 5, 10, 32])
@pytest.mark.parametrize('K', [5, 40, 100])
def test_kernel_matches_restatement_on_reference_log_probs(golden, W, K):
    """the CTC head's log-probs the real reference produced (tests/golden/c1_decode.npz), full and ragged lengths"""
    lp = golden('c1_decode.npz')['ctc_head_logp'].astype(np.float32)        # [4, 35, 100]
    check_against_reference(lp, [35, 35, 35, 35], W, K, min_clear=2)
    check_against_reference(lp, [35, 30, 17, 1], W, K, min_clear=2)


def peaky_log_probs(rng, B, T, V, scale=4.0):
    x = torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * scale)
    return torch.log_softmax(x, -1).numpy()


def test_random_batches_ragged_lengths():
    rng = np.random.default_rng(7)
    B, T, V = 10, 512, 4233
    lp = peaky_log_probs(rng, B, T, V)
    a = 17
    lp[4] = np.log(np.full(V, 1e-6 / (V - 1), np.float32))           # all blank: the empty hypothesis
    lp[4, :, 0] = np.log(1 - 1e-6)
    lp[5, :3] = np.log(np.full(V, 1e-6 / (V - 1), np.float32))       # a, blank, a: the repeat survives as "a a"
    lp[5, [0, 2], a] = np.log(1 - 1e-6)
    lp[5, 1, 0] = np.log(1 - 1e-6)
    lengths = [0, 1, T, 300, 200, 3, 449, 64, 130, 511]
    x = torch.from_numpy(lp).to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    tokens, out_len, scores = ops.ctc_prefix_beam_search(x, ln, beam_width=10, cutoff_top_n=40)
    tokens, out_len, scores = tokens.cpu(), out_len.cpu(), scores.cpu()
    assert out_len[0, 0] == 0 and scores[0, 0] == 0.0 and torch.isinf(scores[0, 1:]).all() and (tokens[0] == -1).all()
    assert out_len[4, 0] == 0 and (tokens[4, 0] == -1).all()
    assert tokens[5, 0, :2].tolist() == [a, a] and out_len[5, 0] == 2
    # utterances 4 and 5 are built from exact ties (gap 0) and checked above; 2 and 6 meet a W/W+1 near-tie (< 1e-4) on the way
    check_against_reference(lp, lengths, 10, 40, min_clear=6)


def test_topk_pass_matches_a_stable_sort():
    """otr_ctc_topk on its own at each register-array size (V <= 1024, <= 4608, <= 8192), ties included"""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for V, K in ((100, 64), (1000, 7), (4233, 40), (4233, 64), (8192, 64), (5000, 1)):
        B, T = 2, 33
        lp = rng.normal(size=(B, T, V)).astype(np.float32)
        lp[0, 0] = np.round(lp[0, 0])                                 # many exact ties, across the K-th value
        lp[0, 1] = -np.inf
        lp[0, 1, 5] = 0.0
        lp[1, 2, :] = -0.0
        lp[1, 2, ::2] = 0.0
        x = torch.from_numpy(lp).to(DEV)
        lengths = torch.tensor([T, T - 3], dtype=torch.int32, device=DEV)
        top_lp = torch.full((B * T, K), 7.0, device=DEV)
        top_tok = torch.full((B * T, K), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.otr_ctc_topk(C.c_void_p(x.data_ptr()), V, C.c_void_p(lengths.data_ptr()), B, T, V, K,
                                    C.c_void_p(top_lp.data_ptr()), C.c_void_p(top_tok.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_ctc_topk')
        got_lp, got_tok = top_lp.cpu().numpy().reshape(B, T, K), top_tok.cpu().numpy().reshape(B, T, K)
        for b in range(B):
            for t in range(T):
                if b == 1 and t >= T - 3:                             # frames past the length are not touched
                    assert (got_tok[b, t] == -7).all() and (got_lp[b, t] == 7.0).all()
                    continue
                want = ref.topk(lp[b, t], K)
                assert got_tok[b, t].tolist() == [v for _, v in want], (V, K, b, t)
                np.testing.assert_array_equal(got_lp[b, t], np.array([p for p, _ in want], np.float32))


def test_brute_force_on_the_device():
    """V = 3, T <= 4, W = 32, K = V: the beam holds every reachable prefix, so every score is the exact CTC log-likelihood of its
    label sequence and the 1-best is the arg-max over all label sequences"""
    rng = np.random.default_rng(11)
    T = 4
    lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(6, T, 3)) * 2.0), -1).numpy().astype(np.float32)
    lengths = [4, 4, 3, 2, 1, 4]
    tokens, out_len, scores = (t.cpu().numpy() for t in ops.ctc_prefix_beam_search(
        torch.from_numpy(lp).to(DEV), torch.tensor(lengths, device=DEV), beam_width=32, cutoff_top_n=3))
    for b, n in enumerate(lengths):
        x = lp[b, :n].astype(np.float64)
        every = {}
        for m in range(n + 1):
            for s in itertools.product([1, 2], repeat=m):
                every[s] = ctc_logprob(x, list(s))
        got = hyps_of(tokens, out_len, scores, b)
        assert set(got) == {s for s, v in every.items() if v > -1e30}
        for s, v in got.items():
            assert abs(v - every[s]) < 1e-5, (b, s, v, every[s])
        assert tuple(tokens[b, 0, :out_len[b, 0]]) == max(every, key=every.get)


def load_c1(g, mode):
    import opentransformer_amd as ota
    ops.set_compute_dtype(mode)
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    return model.to(DEV).eval()


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_recognizer_beam_mode_end_to_end(golden, mode):
    """CTCRecognizer(mode='beam') returns the 1-best of the restatement run on the log-probs assistor.inference produced in the
    same call; at W = 1 with K = V too (which is not greedy decoding in general)"""
    from opentransformer_amd.recognize import CTCRecognizer
    g = golden('c1_decode.npz')
    try:
        model = load_c1(g, mode)
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        seen = []
        inference = model.assistor.inference

        def recording(memory, memory_mask):
            out = inference(memory, memory_mask)
            seen.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
            return out
        model.assistor.inference = recording
        idx2unit = {i: str(i) for i in range(100)}
        for W, K in ((5, 40), (1, 100)):
            rec = CTCRecognizer(model, idx2unit=idx2unit, mode='beam', beam_width=W, cutoff_top_n=K)
            seen.clear()
            got = rec.recognize_beam(x, m)
            lp, ln = seen[0]
            assert lp.dtype == np.float32 and lp.shape == (4, 35, 100)
            gaps = []
            rt, rl, rs = ref.decode(lp, ln, W, K, min_gap=gaps)
            want = [rt[b, 0, :rl[b, 0]].tolist() for b in range(4)]
            for b in range(4):
                if got[b] != want[b]:                                   # only a float32 near-tie may swap the 1-best
                    assert gaps[b] <= 1e-4 or abs(rs[b, 0] - rs[b, 1]) <= 1e-4, (mode, W, b, got[b], want[b])
            assert sum(got[b] == want[b] for b in range(4)) >= 3
            assert rec.recognize(x, m) == rec.translate(got)                 # translate stops at EOS, as in every mode
    finally:
        ops.set_compute_dtype('bf16')


def test_graph_capture_replays_identically():
    """the two launches captured into one graph (a single chain on one stream) and replayed give the eager outputs, also after
    the input buffer is refilled"""
    rng = np.random.default_rng(5)
    B, T, V = 4, 96, 4233
    lp1, lp2 = peaky_log_probs(rng, B, T, V), peaky_log_probs(rng, B, T, V)
    x = torch.from_numpy(lp1).to(DEV)
    ln = torch.tensor([96, 50, 1, 77], dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.load().otr_ctc_beam_workspace_bytes(B, T, 8) // 8, dtype=torch.int64, device=DEV)
    eager1 = [t.clone() for t in ops.ctc_prefix_beam_search(x, ln, beam_width=8, cutoff_top_n=40, workspace=ws)]
    x.copy_(torch.from_numpy(lp2))
    eager2 = [t.clone() for t in ops.ctc_prefix_beam_search(x, ln, beam_width=8, cutoff_top_n=40, workspace=ws)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        out = ops.ctc_prefix_beam_search(x, ln, beam_width=8, cutoff_top_n=40, workspace=ws)
    for lp, want in ((lp1, eager1), (lp2, eager2), (lp1, eager1)):
        x.copy_(torch.from_numpy(lp))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)
