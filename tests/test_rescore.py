"""CPU (-m "not gpu"): attention rescoring of the CTC n-best (SpeechToTextRecognizer rescore=True).  The plain-Python restatement
(tests/rescore_ref.py) on the oracle reproduces what the real reference's decoder and LM give (tests/golden/c1_rescore.npz,
tools/make_rescore_golden.py), has the properties the mode promises, and the recognizer and the library's entry points refuse what is
outside the documented limits before they launch."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from opentransformer_amd import synthetic as syn
from oracle import otrans_oracle as orc
from tests import ctc_prefix_ref, helpers as H, rescore_ref as ref
from tests.test_oracle_golden import _decode_state

EOS = 1


def test_restatement_on_the_oracle_reproduces_the_reference(golden):
    """att(h) / lm(h) of every hypothesis, the totals and the final order of the fixture the real reference produced, within 1e-5
    (fp32 on the CPU on both sides); and no two totals of an utterance within 1e-4 of each other, so tests/test_gpu_rescore.py's
    end-to-end comparison leaves no utterance out on their account"""
    g, base = golden('c1_rescore.npz'), golden('c1_decode.npz')
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    parts = _decode_state(base)
    W, K, max_len = int(g['W']), int(g['K']), int(g['max_len'])
    lm_cfg = syn.lm_config(100, d_model=64, d_ff=128, num_blocks=2)
    lm = (H.lm_state(lm_cfg), lm_cfg)
    with torch.no_grad():
        fe, fm = orc.conv_frontend(parts['frontend'], torch.from_numpy(base['inputs']), torch.from_numpy(base['mask']))
        mem, mm = orc.transformer_encoder(parts['encoder'], fe, fm, cfg['encoder'])
    tokens, out_len, scores = ctc_prefix_ref.decode(base['ctc_head_logp'], mm.sum(-1).tolist(), W, K)
    assert np.array_equal(tokens, g['tokens']) and np.array_equal(out_len, g['out_len'])
    np.testing.assert_allclose(scores, g['scores'], rtol=0, atol=1e-9)
    beam = ref.beam_of(tokens, out_len, scores)
    assert all(any(len(h) > 1 for h, _ in slots) for slots in beam)

    def att_fn(b, h):
        with torch.no_grad():
            return orc.transformer_decoder(parts['decoder'], torch.tensor([[EOS] + list(h)]), mem[b:b + 1], mm[b:b + 1], cfg['decoder'])[0].numpy()

    def lm_fn(b, h):
        p = torch.tensor([[EOS] + list(h)])
        with torch.no_grad():
            return torch.stack([orc.lm_step_log_probs(lm, p[:, :i + 1])[0] for i in range(p.size(1))]).numpy()
    for i, (lam, mu) in enumerate(g['weights'].tolist()):
        got = ref.rescore(beam, att_fn, lam, max_len, lm_fn=lm_fn if mu else None, mu=mu, nbest=W)
        for b, r in enumerate(got):
            live = [w for w in range(W) if r['att'][w] is not None]
            assert live == [w for w in range(W) if g['att'][b, w] > -np.inf]
            np.testing.assert_allclose([r['att'][w] for w in live], g['att'][b, live], rtol=0, atol=1e-5)
            if mu:
                np.testing.assert_allclose([r['lm'][w] for w in live], g['lm'][b, live], rtol=0, atol=1e-5)
            np.testing.assert_allclose(r['total'], g['total_%d' % i][b], rtol=0, atol=1e-5)
            assert r['perm'] == g['perm_%d' % i][b].tolist(), (lam, mu, b)
            t = sorted(x for x in r['total'] if x > -math.inf)
            assert all(y - x > 1e-4 for x, y in zip(t, t[1:])), (lam, mu, b)


def _toy(V=9, seed=0):
    """a beam and 'models' whose logits are deterministic functions of the hypothesis"""
    rng = np.random.default_rng(seed)
    beam = [[((3, 4), -1.0), ((3,), -1.5), ((), -2.0), ((3, 4, 5, 6), -2.5), ((5, 5), -3.0)],
            [((2,), -0.5), ((7, 8, 2), -0.7), ((), -math.inf), ((), -math.inf), ((), -math.inf)]]
    table = {}

    def fn(salt):
        def f(b, h):
            key = (salt, b, tuple(h))
            if key not in table:
                table[key] = rng.normal(size=(len(h) + 1, V)) * 2.0
            return table[key]
        return f
    return beam, fn(0), fn(1)


def test_properties_of_the_restatement():
    beam, att, lm = _toy()
    # W = 1 returns the CTC 1-best
    one = ref.rescore([s[:1] for s in beam], att, 0.3, 8, lm_fn=lm, mu=0.4)
    assert [r['hyps'][0] for r in one] == [beam[0][0][0], beam[1][0][0]]
    # lambda = 1, mu = 0 returns the CTC order
    assert all(r['perm'] == list(range(5)) for r in ref.rescore(beam, att, 1.0, 8, nbest=5))
    # the total is the telescoped joint score of the joint search, (1 - lambda) log P_att + lambda log P_ctc + mu log P_lm, with
    # log P_ctc replaced by the beam's score: log P_att / log P_lm as sums of per-step log-softmaxes of growing prefixes
    lam, mu = 0.3, 0.4
    res = ref.rescore(beam, att, lam, 8, lm_fn=lm, mu=mu, nbest=5)
    for b, slots in enumerate(beam):
        for w, (h, ctc) in enumerate(slots):
            if ctc == -math.inf:
                continue
            tgt = list(h) + [EOS]
            step = lambda f: sum(float(torch.log_softmax(torch.from_numpy(f(b, h)[i]), -1)[t]) for i, t in enumerate(tgt))   # noqa: E731
            assert abs(res[b]['total'][w] - ((1 - lam) * step(att) + lam * ctc + mu * step(lm))) < 1e-9
    # dead slots and hypotheses with len + 1 > max_len sort last, in CTC order
    short = ref.rescore(beam, att, lam, 4, nbest=5)            # (3, 4, 5, 6) needs 5 rows
    assert short[0]['total'][3] == -math.inf and short[0]['perm'][-1] == 3
    assert short[1]['perm'][2:] == [2, 3, 4] and short[1]['scores'][2:] == [-math.inf] * 3
    none = ref.rescore(beam, att, lam, 1, nbest=5)             # only the empty hypothesis fits one row
    assert none[0]['perm'] == [2, 0, 1, 3, 4] and none[1]['perm'] == list(range(5)) and none[1]['scores'] == [-math.inf] * 5
    # exact ties go to the lower CTC rank
    assert ref.order([-2.0, -1.0, -2.0, -math.inf, -1.0]) == [1, 4, 0, 2, 3]


def test_length_penalty_is_the_beam_searchs():
    """total / ((lamda + len) / (lamda + 1)) ** penalty with len = the tokens of h, exactly as SpeechToTextRecognizer._nbest divides"""
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    beam, att, _ = _toy()
    plain = ref.rescore(beam[:1], att, 0.3, 8, nbest=5)[0]
    pen = ref.rescore(beam[:1], att, 0.3, 8, penalty=0.6, lamda=5, nbest=5)[0]
    stub = SimpleNamespace()
    stub.eval = lambda: stub
    rec = SpeechToTextRecognizer(stub, beam_width=5, nbest=5, penalty=0.6, lamda=5, idx2unit={i: str(i) for i in range(9)})
    preds = torch.full((5, 6), EOS, dtype=torch.long)          # BOS (= EOS), the tokens, EOS ...
    for w, (h, _) in enumerate(beam[0]):
        preds[w, 1:1 + len(h)] = torch.tensor(h, dtype=torch.long)
    hyps, scores = rec._nbest(torch.tensor(plain['total'], dtype=torch.float32), preds, 5, 1)
    np.testing.assert_allclose(scores[0].numpy(), np.array(pen['scores']), rtol=1e-6)
    assert [tuple(int(t) for t in s.split()) for s in hyps[0]] == pen['hyps']


def test_pack_restated():
    tokens = -np.ones((1, 3, 6), np.int64)
    tokens[0, 0, :2] = [5, 7]
    tokens[0, 1, :4] = [5, 7, 7, 2]
    ys_in, ys_out, n_rows = ref.pack(tokens, [[2, 4, 0]], [[-1.0, -2.0, -math.inf]], 4, 10)
    assert ys_in.tolist() == [[1, 5, 7, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert ys_out.tolist() == [[5, 7, 1, -1], [-1] * 4, [-1] * 4] and n_rows.tolist() == [3, 0, 0]


def _model(ctc_weight, V=12):
    dec = SimpleNamespace(output_layer=SimpleNamespace(weight=torch.zeros(V, 4)))
    m = SimpleNamespace(decoder=dec, encoder=SimpleNamespace(), eval=lambda: m)
    if ctc_weight > 0:
        m.assistor = SimpleNamespace(blank=0)
    return m


def test_recognizer_refuses_what_rescoring_cannot_do():
    from opentransformer_amd.recognize import SpeechToTextRecognizer, build_recognizer
    ok = SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, rescore=True)
    assert ok.rescore and ok.cutoff_top_n == 40 and not ok.joint_ctc and not ok.apply_cache
    assert not SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4).rescore           # off by default
    with pytest.raises(ValueError, match='assistor'):
        SpeechToTextRecognizer(_model(0.0), ctc_weight=0.3, rescore=True)
    with pytest.raises(ValueError, match='joint_ctc'):
        SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, rescore=True, joint_ctc=True)
    with pytest.raises(ValueError, match='apply_cache'):
        SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, rescore=True, apply_cache=True)
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match='ctc_weight'):
            SpeechToTextRecognizer(_model(0.3), ctc_weight=w, rescore=True)
    with pytest.raises(ValueError, match='W=33'):
        SpeechToTextRecognizer(_model(0.3, V=100), ctc_weight=0.3, beam_width=33, rescore=True)
    with pytest.raises(ValueError, match='nbest'):
        SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, nbest=5, rescore=True)
    with pytest.raises(ValueError, match='V=9000'):
        SpeechToTextRecognizer(_model(0.3, V=9000), ctc_weight=0.3, rescore=True)
    ngram = SimpleNamespace(model_type='ngram')
    ngram.eval = lambda: ngram
    with pytest.raises(ValueError, match='language model'):
        SpeechToTextRecognizer(_model(0.3), lm=ngram, ctc_weight=0.3, rescore=True)
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1, rescore=True)
    assert build_recognizer('speech2text', _model(0.3), None, args, None).rescore
    del args.rescore
    assert not build_recognizer('speech2text', _model(0.3), None, args, None).rescore


def test_entry_points_refuse_bad_arguments():
    """checked on the host before any launch (no GPU needed): W over 32, V over 8192, nbest over W, lambda outside [0, 1]"""
    from opentransformer_amd import ops
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def select(W=5, nbest=2, lam=0.3, B=2, T=10):
        return lib.otr_rescore_select(p, p, p, p, p, None, B, W, T, nbest, lam, 0.0, 0.0, 5.0, p, p, p, p, p, None)
    assert select(W=33) != 0 and b'rescore_select' in lib.otr_last_error_string()
    assert select(W=0) != 0 and select(nbest=6) != 0 and select(nbest=0) != 0
    assert select(lam=1.5) != 0 and select(lam=-0.5) != 0 and select(lam=float('nan')) != 0
    assert select(B=0) != 0 and select(T=0) != 0
    assert lib.otr_rescore_score(p, 9000, None, 0, p, 8, p, 4, 8, 9000, p, None, None) != 0        # V > 8192
    assert lib.otr_rescore_score(p, 90, None, 0, p, 8, p, 4, 8, 100, p, None, None) != 0           # ld < V
    assert lib.otr_rescore_score(p, 100, p, 100, p, 8, p, 4, 8, 100, p, None, None) != 0           # LM logits without an output
    assert lib.otr_rescore_score(p, 100, None, 0, p, 7, p, 4, 8, 100, p, None, None) != 0          # target rows shorter than max_len
    assert b'rescore_score' in lib.otr_last_error_string()
    assert lib.otr_rescore_pack(p, p, p, 4, 10, 8, 9000, 1, 1, p, p, p, None) != 0                 # V > 8192
    assert lib.otr_rescore_pack(p, p, p, 4, 10, 0, 100, 1, 1, p, p, p, None) != 0                  # max_len < 1
    assert lib.otr_rescore_pack(p, p, p, 4, 10, 8, 100, 100, 1, p, p, p, None) != 0                # BOS outside the vocabulary
    ln0 = _lib.DecLn(None, 16, None, 0, None, None, None, None, 0.0, 1e-5, 0, None, None, None, None, None)
    one = C.c_void_p(16)
    assert lib.otr_dec_cross_fwd_shared(C.byref(ln0), 10, 8, one, one, one, one, 512, 512, 0, 256, None, 4, 3, one, one, one, one, None) != 0
    assert b'share' in lib.otr_last_error_string()                                                 # 10 sequences, 3 per memory
    # the Python entries refuse before they look at the device (CPU tensors here)
    tok, n, sc = torch.zeros((2, 5, 7), dtype=torch.long), torch.zeros((2, 5), dtype=torch.int32), torch.zeros(2, 5)
    lg = torch.zeros(2 * 5 * 4, 100)
    for kw, pat in ((dict(ctc_weight=1.2), 'ctc_weight'), (dict(ctc_weight=0.3, nbest=6), 'nbest'), (dict(ctc_weight=0.3, V=9000), 'V=9000')):
        kw = dict(dict(V=100), **kw)
        with pytest.raises(ValueError, match=pat):
            ops.attention_rescore(lg, tok, n, sc, 4, **kw)
    with pytest.raises(ValueError, match='W=33'):
        ops.attention_rescore(lg, torch.zeros((2, 33, 7), dtype=torch.long), n, sc, 4, 100, 0.3)
    with pytest.raises(ValueError, match='V=9000'):
        ops.rescore_pack(tok, n, sc, 4, 9000)
    with pytest.raises(_lib.OtransHipError):                   # and there is no CPU fallback
        ops.attention_rescore(lg, tok, n, sc, 4, 100, 0.3)
