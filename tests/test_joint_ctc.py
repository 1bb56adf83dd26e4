"""CPU (-m "not gpu"): the joint CTC/attention beam search (SpeechToTextRecognizer joint_ctc=True).  The plain-Python restatement
(tests/ctc_prefix_score_ref.py) has the CTC prefix score of brute force and torch's CTC loss, reduces to the plain search at
lambda = 0, and the recognizer and the library's entry points refuse what is outside the documented limits before they launch."""
import ctypes as C
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opentransformer_amd import _lib
from tests import ctc_prefix_score_ref as ref

BLANK, EOS = 0, 1


def rand_lp(rng, T, V, peak=2.0):
    lp = rng.normal(size=(T, V)) * peak
    return (lp - np.log(np.exp(lp).sum(-1, keepdims=True))).tolist()


def collapse(path):
    out, last = [], None
    for c in path:
        if c != last and c != BLANK:
            out.append(c)
        last = c
    return out


@pytest.mark.parametrize('T,V', [(1, 3), (2, 4), (4, 3), (5, 4), (6, 3), (6, 4)])
def test_prefix_score_is_the_brute_force_prefix_probability(T, V):
    """psi(h) = log of the probability mass of every alignment whose collapsed output starts with h (all V^T alignments); EOS: the
    output equals g (-ctc_loss).  Prefixes g over the tokens 2 .. V-1 (1 is EOS), with repeats."""
    rng = np.random.default_rng(10 * T + V)
    x = rand_lp(rng, T, V)
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        p = math.exp(sum(x[t][c] for t, c in enumerate(path)))
        key = tuple(collapse(path))
        mass[key] = mass.get(key, 0.0) + p
    toks = list(range(2, V))
    for n in range(0, min(T, 3) + 1):
        for g in itertools.product(toks, repeat=n):
            got = ref.prefix_scores(x, T, list(g), list(range(V)), BLANK, EOS)
            assert got[BLANK] == -math.inf
            for c in toks:
                h = g + (c,)
                want = sum(m for k, m in mass.items() if k[:len(h)] == h)
                if want == 0.0:
                    assert got[c] == -math.inf, (g, c)
                else:
                    assert abs(got[c] - math.log(want)) < 1e-9, (g, c, got[c], math.log(want))
            # EOS: log P(output == g) by torch's CTC loss (-inf where g cannot fit)
            if n == 0:
                want = math.log(mass.get((), 0.0)) if mass.get((), 0.0) > 0 else -math.inf
            else:
                nll = F.ctc_loss(torch.tensor(x, dtype=torch.float64).unsqueeze(1), torch.tensor([list(g)]), torch.tensor([T]),
                                 torch.tensor([n]), blank=BLANK, reduction='none', zero_infinity=False)
                want = -float(nll[0])
            if want == -math.inf or want < -1e29:
                assert got[EOS] == -math.inf or got[EOS] < -1e29
            else:
                assert abs(got[EOS] - want) < 1e-9, (g, got[EOS], want)


def toy_models(V, seed):
    """an 'attention decoder' and an 'LM' whose log-probs are deterministic functions of the prefix"""
    def fn(salt, scale):
        def f(preds):
            rows = []
            for row in preds.tolist():
                g = torch.Generator().manual_seed(hash((seed, salt) + tuple(row)) & 0x7fffffff)
                rows.append(torch.log_softmax(torch.randn(V, generator=g) * scale, -1))
            return torch.stack(rows)
        return f
    return fn(1, 3.0), fn(2, 1.0)


@pytest.mark.parametrize('with_lm', [False, True])
def test_restated_joint_search_at_lambda_zero_is_the_plain_search(with_lm):
    V, B, beam = 12, 3, 4
    rng = np.random.default_rng(5)
    att, lm = toy_models(V, 7)
    joint = dict(x=[rand_lp(rng, 9, V) for _ in range(B)], lengths=[9, 4, 1], ctc_weight=0.0, K=6, blank=BLANK)
    kw = dict(lm_fn=lm if with_lm else None, lm_weight=0.4 if with_lm else 0.0, nbest=beam)
    h0, s0 = ref.beam_search(att, B, beam, 8, EOS, **kw)
    h1, s1 = ref.beam_search(att, B, beam, 8, EOS, joint=joint, **kw)
    assert h0 == h1
    assert torch.equal(s0, s1)
    # and a lambda > 0 changes the search (the CTC head is consulted)
    joint['ctc_weight'] = 0.7
    h2, _ = ref.beam_search(att, B, beam, 8, EOS, joint=joint, **kw)
    assert h2 != h0


def _model(ctc_weight, V=12):
    enc = SimpleNamespace()
    dec = SimpleNamespace(output_layer=SimpleNamespace(weight=torch.zeros(V, 4)))
    m = SimpleNamespace(decoder=dec, encoder=enc, eval=lambda: m)
    if ctc_weight > 0:
        m.assistor = SimpleNamespace(blank=0)
    return m


def test_recognizer_refuses_what_the_joint_search_cannot_do():
    from opentransformer_amd.recognize import SpeechToTextRecognizer, build_recognizer
    ok = SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, joint_ctc=True)
    assert ok.ctc_beam == 6                                        # min(V, int(1.5 * beam))
    assert SpeechToTextRecognizer(_model(0.3, V=5), ctc_weight=0.3, beam_width=4, joint_ctc=True).ctc_beam == 5
    plain = SpeechToTextRecognizer(_model(0.0), ctc_weight=0.7, beam_width=4)   # the default: ctc_weight accepted and unused
    assert not plain.joint_ctc
    with pytest.raises(ValueError, match='assistor'):
        SpeechToTextRecognizer(_model(0.0), ctc_weight=0.3, joint_ctc=True)
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match='ctc_weight'):
            SpeechToTextRecognizer(_model(0.3), ctc_weight=w, joint_ctc=True)
    with pytest.raises(ValueError, match='beam_width'):
        SpeechToTextRecognizer(_model(0.3, V=100), ctc_weight=0.3, beam_width=17, joint_ctc=True)
    with pytest.raises(ValueError, match='ctc_beam'):
        SpeechToTextRecognizer(_model(0.3, V=100), ctc_weight=0.3, beam_width=4, ctc_beam=33, joint_ctc=True)
    with pytest.raises(ValueError, match='ctc_beam'):
        SpeechToTextRecognizer(_model(0.3, V=100), ctc_weight=0.3, beam_width=4, ctc_beam=3, joint_ctc=True)
    with pytest.raises(ValueError, match='ctc_beam'):
        SpeechToTextRecognizer(_model(0.3, V=8), ctc_weight=0.3, beam_width=4, ctc_beam=9, joint_ctc=True)
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1,
                           joint_ctc=True, ctc_beam=5)
    rec = build_recognizer('speech2text', _model(0.3), None, args, None)
    assert rec.joint_ctc and rec.ctc_beam == 5
    del args.joint_ctc, args.ctc_beam
    assert not build_recognizer('speech2text', _model(0.3), None, args, None).joint_ctc


def test_entry_points_refuse_bad_arguments():
    """checked on the host before any launch (no GPU needed): K' over 32 or V, T' over 2048, beam over 16 or K', lambda outside [0, 1]"""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.otr_joint_prebeam(p, 100, None, 0, 1.0, 0.0, 4, 100, 33, p, p, None) != 0
    assert lib.otr_joint_prebeam(p, 100, None, 0, 1.0, 0.0, 4, 10, 11, p, p, None) != 0
    assert lib.otr_joint_prebeam(p, 9000, None, 0, 1.0, 0.0, 4, 9000, 8, p, p, None) != 0

    def ps(T=50, V=100, K=8, beam=4, lam=0.3, cand_score=p):
        return lib.otr_ctc_prefix_score(p, V, p, 1, T, V, 0, 1, 4, 4, K, p, cand_score, None, p, 10, 1, None, p, p, p, p, lam, p, p, p,
                                        beam, p, p, p, None)
    assert ps(T=2049) != 0
    assert ps(K=33) != 0
    assert ps(beam=17, K=20) != 0
    assert ps(beam=9, K=8) != 0
    assert ps(lam=1.5) != 0 and ps(lam=-0.5) != 0
    assert b'ctc_prefix_score' in lib.otr_last_error_string()
    one = [p] * 5
    assert lib.otr_beam_prune_joint(*one, 10, 1, 17, 1, 1, *([p] * 6), None) != 0
