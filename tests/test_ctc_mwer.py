"""CPU (-m "not gpu"): minimum word error rate training of the CTC model.  The numpy float64 restatement (tests/ctc_mwer_ref.py) agrees
with an independent composition from torch ops and with its own central differences and has the properties the loss promises; the
library's entry points, ops.ctc_mwer_loss and CTCMWERTraining refuse what is outside the documented limits before they launch."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import opentransformer_amd as ota
from opentransformer_amd import _lib
from opentransformer_amd import synthetic as syn
from opentransformer_amd.mwer import CTCMWERTraining       # noqa: F401  (the feature: without it nothing in this file has a subject)
from opentransformer_amd.ops import ctc_mwer_loss          # noqa: F401
from tests import ctc_mwer_cases as cases
from tests import ctc_mwer_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def _args(c, with_ref=True):
    return (c['logits'], c['in_len'], c['hyps'], c['hyp_len'], c['errors']) + ((c['ref'], c['ref_len']) if with_ref else (None, None))


@pytest.mark.parametrize('V', [7, 100, 4233])
@pytest.mark.parametrize('N', [2, 5, 32])
def test_restatement_matches_the_torch_composition(V, N):
    """float64 on both sides; the bounds tests/test_mwer.py holds mwer_ref to: 1e-12 on the values, 1e-8 on the gradient"""
    main = cases.main_case(100 * N + V, 4, 40, V, N)
    edged, dead = cases.with_edges(main, V)
    for c, dead_c in ((main, np.zeros_like(dead)), (edged, dead)):
        for w, scale, with_ref in ((0.0, 1.0, False), (0.3, 1.0, True), (0.3, 0.1, True)):
            f = ref.forward(*_args(c, with_ref), ctc_weight=w, scale=scale)
            assert np.array_equal(f['live'], ~dead_c)
            loss, mwer, ctc, d = cases.compose_torch(c, f['live'], w, scale, with_ref)
            assert abs(f['loss'] - loss.item()) < 1e-12 * max(1, abs(f['loss'])) and abs(f['mwer'] - mwer.item()) < 1e-12 * max(1, f['mwer'])
            assert abs(f['ctc'] - ctc.item()) < 1e-12 * max(1, f['ctc'])
            g = ref.grad(*_args(c, with_ref), ctc_weight=w, scale=scale)
            assert np.abs(g).max() > 1e-4 and np.abs(g - d).max() < 1e-8


@pytest.mark.parametrize('N', [2, 5])
def test_restatement_matches_its_finite_differences(N):
    V = 23
    c, _ = cases.with_edges(cases.main_case(N, 4, 40, V, N), V)
    rng = np.random.default_rng(N)
    picks = []
    for _ in range(60):                                       # label and blank columns of live frames among them
        b = int(rng.integers(3))
        t = int(rng.integers(c['in_len'][b]))
        v = int(c['ref'][b, 0]) if rng.random() < 0.3 else (0 if rng.random() < 0.2 else int(rng.integers(V)))
        picks.append((b, t, v))
    assert ref.finite_difference_error(picks, *_args(c), ctc_weight=0.3, scale=1.0) < 1e-8
    assert ref.finite_difference_error(picks, *_args(c, False), scale=0.1) < 1e-8


def test_one_hypothesis_or_equal_errors_give_the_errors_and_no_gradient():
    V = 17
    c = cases.main_case(0, 4, 40, V, 1)
    c['errors'][:, 0] = [3, 0, 2, 7]
    f = ref.forward(*_args(c, False))
    assert f['loss'] == 3.0 and not ref.grad(*_args(c, False)).any()          # exactly: P = 1, W - E = 0
    c = cases.main_case(1, 4, 40, V, 4)
    c['errors'][:] = 3
    f = ref.forward(*_args(c, False))
    assert abs(f['loss'] - 3.0) < 1e-12 and np.abs(f['c']).max() < 1e-15 and np.abs(ref.grad(*_args(c, False))).max() < 1e-15


@pytest.mark.parametrize('V', [7, 100])
def test_the_softmax_term_cancels(V):
    """autograd knows nothing of the cancellation: its MWER gradient sums to zero along every row and vanishes off the columns of the
    hypotheses' labels and of the blank, which is where the restatement (and the kernel) put nothing at all"""
    N = 5
    c, _ = cases.with_edges(cases.main_case(V, 4, 40, V, N), V)
    f = ref.forward(*_args(c, False))
    _, _, _, d = cases.compose_torch(c, f['live'], 0.0, 1.0, False)
    g = ref.grad(*_args(c, False))
    # the restatement forms every occupancy as exp(alpha + beta - lp - ll): the exponent is a difference of numbers as large as |ll|,
    # so it carries a few roundings of |ll| * 2^-52, and the occupancy that relative error; |c| < 1 and the rows of gamma sum to 1
    floor = 8 * np.abs(f['seq_logp'][f['live']]).max() * 2.0 ** -52
    assert np.abs(d).max() > 1e-4 and np.abs(d.sum(axis=-1)).max() < 1e-15 and np.abs(g.sum(axis=-1)).max() < floor < 1e-12
    for b in range(4):
        cols = np.zeros(V, bool)
        cols[cases.BLANK] = True
        for n in range(N):
            if f['live'][b, n]:
                cols[c['hyps'][b, n, :c['hyp_len'][b, n]]] = True
        assert not g[b][:, ~cols].any() and not g[b, c['in_len'][b]:].any()
        if V > 7:
            assert (~cols).any() and np.abs(d[b][:, ~cols]).max() < floor      # softmax * sum_n c_n, every c_n through exp(ll_n)


def test_dead_slots_and_dead_utterances():
    V, N = 11, 5
    main = cases.main_case(3, 4, 40, V, N)
    base = ref.forward(*_args(main))
    assert base['b_live'] == 4 and base['live'].all()
    c, dead = cases.with_edges(main, V)
    assert c['errors'][1, 4] < 0 and c['hyp_len'][1, 3] == 128 and c['hyps'][1, 2, 1] >= V and c['hyp_len'][2, 4] > c['in_len'][2] > 0
    assert c['in_len'][3] == 0 and c['hyp_len'][0, 3] == 0 and c['hyps'][0, 4, 0] == c['hyps'][0, 4, 1]
    f = ref.forward(*_args(c))
    assert np.array_equal(f['live'], ~dead) and f['b_live'] == 3
    assert not f['post'][dead].any() and np.all(f['seq_logp'][dead] == -np.inf) and f['utt_err'][3] == 0
    assert np.allclose(f['post'][:3].sum(axis=1), 1) and np.isfinite(f['seq_logp'][0, 3])     # the empty hypothesis is live
    assert abs(f['mwer'] - f['utt_err'][:3].sum() / 3) < 1e-12
    g = ref.grad(*_args(c), ctc_weight=0.3)
    assert not g[3].any() and f['nll_ref'][3] == 0 and not f['ok_ref'][3]
    # a length of 128 in rows that are wide enough: the bound of 127 kills it, not the width
    big, dead = cases.big_case()
    f = ref.forward(*_args(big))
    assert big['hyps'].shape[2] >= 128 and np.array_equal(f['live'], ~dead) and cases.carrying_share(big) == 1.0
    # every slot dead: nothing is live, the loss is the CTC term alone
    c['errors'][:] = -1
    f = ref.forward(*_args(c), ctc_weight=0.3)
    assert f['b_live'] == 0 and f['mwer'] == 0 and f['loss'] == 0.3 * f['ctc'] > 0


# ---------------------------------------------------------------- the library and the ops, without a device
def test_abi_version_is_still_608_and_the_header_names_both_entries():
    header = (ROOT / 'include' / 'otrans_hip.h').read_text()
    assert re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1) == '608' and _lib.OTR_ABI_VERSION == 608
    still = header[header.index('still 608'):header.index('#define OTR_ABI_VERSION')]
    for name in ('otr_ctc_mwer_workspace_floats', 'otr_ctc_mwer_loss'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SIGNATURES and name in still
        for kind in ('bf16', 'fp16'):
            lib = _lib.load(kind)
            assert lib.otr_version() == 608 and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES['otr_ctc_mwer_loss']) == 27


def test_workspace_size_and_bad_shapes():
    lib = _lib.load()
    assert lib.otr_ctc_mwer_workspace_floats(32, 4, 250, 20) == 5 * 32 * 250 * 41 + 32 * 5
    assert lib.otr_ctc_mwer_workspace_floats(1, 1, 1, 0) == 2 + 2
    for B, N, T, mt in ((0, 4, 9, 8), (65536, 4, 9, 8), (4, 0, 9, 8), (4, 33, 9, 8), (4, 4, 0, 8), (4, 4, 9, -1), (4, 4, 9, 128)):
        assert lib.otr_ctc_mwer_workspace_floats(B, N, T, mt) == -1, (B, N, T, mt)


def test_entry_point_refuses_bad_arguments_and_leaves_the_outputs_alone():
    """checked on the host before any launch (no GPU needed): every output buffer still holds its fill afterwards"""
    lib = _lib.load()
    fill = 123.25
    bufs = {k: (C.c_float * 64)(*([fill] * 64)) for k in ('loss3', 'seq', 'post', 'utt', 'nll', 'dl', 'ws')}
    p = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}
    inp = C.cast((C.c_float * 64)(), C.c_void_p)
    need = lib.otr_ctc_mwer_workspace_floats(2, 4, 10, 8)

    def call(lp=inp, in_len=inp, hyps=inp, ldh=8, hyp_len=inp, errors=inp, rf=inp, ldr=8, ref_len=inp, w=0.3, scale=1.0, B=2, N=4,
             T=10, V=100, mt=8, blank=0, loss3=p['loss3'], seq=p['seq'], post=p['post'], utt=p['utt'], nll=p['nll'], dl=p['dl'],
             ws=p['ws'], nws=need):
        return lib.otr_ctc_mwer_loss(lp, in_len, hyps, ldh, hyp_len, errors, rf, ldr, ref_len, w, scale, None, B, N, T, V, mt, blank,
                                     loss3, seq, post, utt, nll, dl, ws, nws, None)
    inf, nan = float('inf'), float('nan')
    bad = [dict(lp=None), dict(in_len=None), dict(hyps=None), dict(hyp_len=None), dict(errors=None), dict(loss3=None), dict(seq=None),
           dict(post=None), dict(utt=None), dict(nll=None), dict(ws=None),
           dict(rf=None), dict(ref_len=None), dict(rf=None, ref_len=None), dict(rf=None, ldr=0), dict(ref_len=None, ldr=0),
           dict(B=0), dict(B=65536), dict(N=0), dict(N=33), dict(T=0), dict(V=1), dict(mt=-1), dict(mt=128, ldh=128, ldr=128),
           dict(ldh=7), dict(ldr=7), dict(blank=-1), dict(blank=100), dict(w=-0.1), dict(w=inf), dict(w=nan), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=inf), dict(scale=nan), dict(nws=need - 1)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b'ctc_mwer_loss' in lib.otr_last_error_string(), kw
    for k, b in bufs.items():
        assert all(v == fill for v in b), k


def _cpu_args(B=2, N=3, T=12, V=10, L=5):
    return dict(logits=torch.zeros(B, T, V), in_len=torch.full((B,), T), hyps=torch.ones((B, N, L), dtype=torch.long),
                hyp_len=torch.full((B, N), 2, dtype=torch.int32), errors=torch.zeros((B, N), dtype=torch.int32))


def test_ops_refuse_before_they_look_at_the_device():
    from opentransformer_amd import loss_ops, ops
    assert ops.ctc_mwer_loss is loss_ops.ctc_mwer_loss and ops.CtcMwerLossFn is loss_ops.CtcMwerLossFn
    a = _cpu_args()
    with pytest.raises(_lib.OtransHipError):                   # CPU tensors: there is no fallback
        ops.ctc_mwer_loss(**a)
    ref_rows, ref_len = torch.ones((2, 4), dtype=torch.long), torch.full((2,), 3)
    for kw, match in ((dict(logits=torch.zeros(2, 12)), 'logits must be'), (dict(logits=torch.zeros(2, 12, 1)), 'V >= 2'),
                      (dict(hyps=a['hyps'][0]), 'hyps must be'), (dict(errors=a['errors'].view(-1)), 'hyps must be'),
                      (dict(hyp_len=a['hyp_len'][:1]), 'hyps must be'), (dict(in_len=a['in_len'][:1]), 'in_len'),
                      (dict(ref=ref_rows), 'go together'), (dict(ref_len=ref_len), 'go together'),
                      (dict(ref=ref_rows[:1], ref_len=ref_len), 'ref must be'), (dict(ref=ref_rows, ref_len=ref_len[:1]), 'ref_len'),
                      (dict(ref=torch.ones((2, 128), dtype=torch.long), ref_len=ref_len), 'width 128'),
                      (dict(ctc_weight=-1.0), 'ctc_weight'), (dict(ctc_weight=float('nan')), 'ctc_weight'), (dict(scale=0.0), 'scale'),
                      (dict(scale=float('inf')), 'scale'), (dict(blank=10), 'blank'), (dict(blank=-1), 'blank')):
        with pytest.raises(ValueError, match=match):
            ops.ctc_mwer_loss(**dict(a, **kw))
    big = _cpu_args(N=33)
    with pytest.raises(ValueError, match='N=33'):
        ops.ctc_mwer_loss(**big)


def _models():
    cfg = syn.c1_model(0.0)
    return ota.CTCModel(dict(cfg, vocab_size=cfg['decoder']['vocab_size'])), ota.SpeechToText(cfg), cfg


def test_trainer_checks_and_is_a_model_training():
    from opentransformer_amd import model as M
    from opentransformer_amd.recognize import CTCRecognizer
    ctc, s2t, cfg = _models()
    ctc.train()
    modes = [m.training for m in ctc.modules()]
    wrap = ota.CTCMWERTraining(ctc, nbest=3, cutoff_top_n=20)
    assert isinstance(wrap, M.ModelTraining) and wrap.model is ctc and [m.training for m in ctc.modules()] == modes
    rec = wrap.recognizer
    assert isinstance(rec, CTCRecognizer) and rec.mode == 'beam' and rec.beam_width == 3 and rec.cutoff_top_n == 20
    assert ota.CTCMWERTraining(ctc, nbest=2, beam_width=6).recognizer.beam_width == 6
    assert [n for n, _ in wrap.named_parameters()] == ['model.' + n for n, _ in ctc.named_parameters()]
    with pytest.raises(TypeError, match='CTCModel'):
        ota.CTCMWERTraining(s2t)
    with pytest.raises(TypeError, match='CTCMWERTraining'):     # the attention trainer names the class to use instead
        ota.MWERTraining(ctc)
    for kw, match in ((dict(nbest=0), 'nbest'), (dict(nbest=33), 'nbest'), (dict(nbest=4, beam_width=2), 'beam_width'),
                      (dict(ctc_weight=-1), 'ctc_weight'), (dict(scale=0), 'scale'), (dict(scale=float('nan')), 'scale')):
        with pytest.raises(ValueError, match=match):
            ota.CTCMWERTraining(ctc, **kw)
    inputs, targets = syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=cfg['decoder']['vocab_size'],
                                          tgt_len=4, seed=0)
    with pytest.raises(ValueError, match='hyps must be'):
        wrap(inputs, targets, hyps=(torch.ones((2, 5), dtype=torch.long), torch.ones(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match='33 hypotheses'):
        wrap(inputs, targets, hyps=(torch.ones((2, 33, 5), dtype=torch.long), torch.ones((2, 33), dtype=torch.int32)))


def test_trainer_arrives_at_the_one_encode_step(monkeypatch):
    """tests/test_model_passes.py's spy: with the hypotheses given, the first thing that touches the model is AcousticModel.encode,
    unmarked, as for every CTCModel pass"""
    from opentransformer_amd import model as M
    from opentransformer_amd import ops
    ctc, _, cfg = _models()
    wrap = ota.CTCMWERTraining(ctc, nbest=2)
    inputs, targets = syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=cfg['decoder']['vocab_size'],
                                          tgt_len=4, seed=0)
    seen = []

    class Reached(Exception):
        pass

    def spy(self, inputs, inputs_mask, mark=False):
        seen.append((type(self).__name__, mark))
        raise Reached()
    monkeypatch.setattr(M.AcousticModel, 'encode', spy)
    monkeypatch.setattr(ops, 'edit_distance', lambda r, rl, h, hl: (torch.zeros(h.shape[:2], dtype=torch.int32),))
    with pytest.raises(Reached):
        wrap(inputs, targets, hyps=(torch.ones((2, 2, 5), dtype=torch.long), torch.ones((2, 2), dtype=torch.int32)))
    assert seen == [('CTCModel', False)]
