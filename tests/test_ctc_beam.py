"""CPU (-m "not gpu"): the CTC prefix beam search.  The plain-Python restatement (tests/ctc_prefix_ref.py) is exact when the beam
holds every reachable prefix (checked against torch's CTC loss and brute force), keeps the documented tie order, and the library's
entry points refuse bad arguments before they launch (no GPU here)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opentransformer_amd import _lib
from tests import ctc_prefix_ref as ref


def ctc_logprob(lp, label):
    """log P(label | lp) by torch's CTC loss (blank 0), lp [T, V] float64"""
    x = torch.from_numpy(lp).unsqueeze(1)
    tg = torch.tensor([label if label else [1]], dtype=torch.long)
    nll = F.ctc_loss(x, tg, torch.tensor([lp.shape[0]]), torch.tensor([len(label)]), blank=0, reduction='none',
                     zero_infinity=False)
    return -float(nll[0])


@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_is_exact_when_the_beam_holds_every_prefix(T, seed):
    """V = 3 (blank + 2 tokens), T <= 4: at most 31 label sequences, all of them fit a beam of 32 with K = V"""
    rng = np.random.default_rng(100 * T + seed)
    lp = rng.normal(size=(T, 3)) * 2.0
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    hyps = ref.decode_one(lp, T, W=32, K=3)
    got = {s: sc for s, sc in hyps}
    for s, sc in got.items():
        assert abs(sc - ctc_logprob(lp, list(s))) < 1e-5, s
    every = {}
    for n in range(T + 1):
        for s in itertools.product([1, 2], repeat=n):
            v = ctc_logprob(lp, list(s))
            if v > -1e30:
                every[s] = v
    assert set(got) == set(every)                                  # every reachable sequence, nothing else
    best = max(every, key=every.get)
    assert hyps[0][0] == best
    assert [sc for _, sc in hyps] == sorted((sc for _, sc in hyps), reverse=True)


def test_reference_collapse_rules_and_padding():
    V, NEG = 4, -30.0
    def frames(*toks):
        lp = np.full((len(toks), V), NEG)
        for t, c in enumerate(toks):
            lp[t, c] = 0.0
        return lp
    tokens, out_len, scores = ref.decode(np.stack([frames(2, 0, 2), frames(2, 2, 2), frames(0, 0, 0)]), [3, 3, 3], W=3, K=4)
    assert tokens[0, 0].tolist() == [2, 2, -1] and out_len[0, 0] == 2          # a blank splits a repeat
    assert tokens[1, 0].tolist() == [2, -1, -1] and out_len[1, 0] == 1         # repeats collapse
    assert out_len[2, 0] == 0 and tokens[2, 0].tolist() == [-1, -1, -1]        # all blank: the empty hypothesis
    assert abs(scores[2, 0]) < 1e-9
    t1, l1, s1 = ref.decode(frames(1, 2)[None], [0], W=4, K=2)                 # zero frames: the empty prefix alone
    assert l1[0].tolist() == [0, 0, 0, 0] and s1[0, 0] == 0.0 and np.isinf(s1[0, 1:]).all()


def test_reference_tie_order():
    """equal scores: lower parent slot first, then lower token; a carried-over prefix counts as token -1"""
    lp = np.log(np.full((1, 4), 0.25))
    hyps = ref.decode_one(lp, 1, W=4, K=4)
    assert [s for s, _ in hyps] == [(), (1,), (2,), (3,)]
    assert ref.topk(np.array([0.5, 0.7, 0.7, 0.1]), 2) == [(0.7, 1), (0.7, 2)]


def test_ctc_beam_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    al = C.c_void_p(4096)
    B, T, V = 2, 8, 100
    ws = lib.otr_ctc_beam_workspace_bytes(B, T, 5)
    assert ws == B * T * 5 * 8
    assert lib.otr_ctc_beam_workspace_bytes(B, T, 0) < 0 and lib.otr_ctc_beam_workspace_bytes(B, T, 33) < 0

    def search(W=5, K=40, blank=0, V=V, ws_bytes=ws, workspace=al):
        return lib.otr_ctc_beam_search(al, al, al, B, T, V, K, blank, W, workspace, ws_bytes, al, al, al, None)

    def topk(K=40, V=V, ld=V):
        return lib.otr_ctc_topk(al, ld, al, B, T, V, K, al, al, None)
    assert search(W=0) < 0 and b'ctc_beam_search' in lib.otr_last_error_string()
    assert search(W=33) < 0
    assert search(K=129, V=200) < 0 and search(K=0) < 0
    assert search(K=40, V=30) < 0 and search(K=101) < 0                # K > V
    assert search(blank=V) < 0 and search(blank=-1) < 0
    assert search(ws_bytes=ws - 1) < 0 and b'workspace' in lib.otr_last_error_string()
    assert search(workspace=C.c_void_p(4096 + 4)) < 0                # misaligned workspace
    assert topk(K=129, V=200, ld=200) < 0 and b'ctc_topk' in lib.otr_last_error_string()
    assert topk(K=0) < 0 and topk(K=40, V=30, ld=30) < 0
    assert topk(V=8193, ld=8193) < 0 and topk(ld=V - 1) < 0


def test_ctc_beam_op_refuses_cpu_tensors():
    from opentransformer_amd import ops
    with pytest.raises(_lib.OtransHipError):
        ops.ctc_prefix_beam_search(torch.zeros(1, 4, 5), torch.tensor([4]))


def test_ctc_recognizer_accepts_beam_mode_and_refuses_an_ngram_lm():
    import opentransformer_amd as ota
    from opentransformer_amd import synthetic as syn
    from opentransformer_amd.recognize import CTCRecognizer
    model = ota.SpeechToText(syn.c1_model(ctc_weight=0.3))
    rec = CTCRecognizer(model, mode='beam', beam_width=5, alpha=0.5, beta=1.0)
    assert rec.mode == 'beam' and rec.beam_width == 5
    with pytest.raises(NotImplementedError):
        CTCRecognizer(model, mode='beam', ngram_lm='lm.arpa')
    with pytest.raises(NotImplementedError):
        CTCRecognizer(model, mode='sampling')
