"""CPU (-m "not gpu"): the restatement of the transducer's beam search (tests/rnnt_beam_ref.py) against the enumeration of every
alignment of the one-symbol-per-frame lattice, its edge cases, and the host side of the feature: the refusals of ops.rnnt_beam, of
the entries and of TransducerRecognizer (raised before the device is touched), and the registries."""
import ctypes as C
import math
import types

import pytest
import torch

from opentransformer_amd import _lib, loss_ops, ops
from tests import rnnt_beam_ref as br
from tests import rnnt_cases as rc
from tests import rnnt_ref as rr


@pytest.fixture(autouse=True)
def the_search_the_restatement_restates():
    """every test here is about ops.rnnt_beam: the restatement alone, without the search it states, checks nothing of the package"""
    assert callable(getattr(ops, 'rnnt_beam', None)) and 'otr_rnnt_beam_select' in _lib.SIGNATURES


def _table(T=3, **kw):
    pe, table, weight, bias = br.table_model(V=3, J=4, T=T, **kw)
    return (pe,) + br.table_callbacks(table, weight, bias)


def test_every_hypothesis_scores_the_sum_of_its_alignments():
    """V 3, T 3, W 16: all 15 sequences fit, so nothing is pruned and every score is the log-sum over the enumerated alignments (27
    paths) -- which holds only if identical hypotheses were merged"""
    pe, predict, joint = _table()
    hyps, gap, merges = br.rnnt_beam_ref(pe, 3, predict, joint, 16, 50)
    want = br.enumerate_ref(pe, 3, predict, joint, 3)
    assert len(want) == 15 and len(hyps) == 15 and merges >= 1
    assert sorted(tuple(h[0]) for h in hyps) == sorted(want)
    assert abs(math.log(sum(math.exp(v) for v in want.values()))) < 1e-12          # the 27 paths are a distribution
    for y, fr, s in hyps:
        assert abs(s - want[tuple(y)]) <= 1e-12, (y, s, want[tuple(y)])
        assert len(fr) == len(y) and fr == sorted(set(fr)) and all(0 <= f < 3 for f in fr)      # one symbol per frame at most
    assert [h[2] for h in hyps] == sorted((h[2] for h in hyps), reverse=True)


def test_max_len_truncates_and_keeps_the_sum_over_the_alignments_that_fit():
    pe, predict, joint = _table(seed=1)
    hyps, _, merges = br.rnnt_beam_ref(pe, 3, predict, joint, 16, 2)
    want = br.enumerate_ref(pe, 3, predict, joint, 3, max_len=2)
    assert len(want) == 7 and sorted(tuple(h[0]) for h in hyps) == sorted(want) and merges >= 1
    assert max(len(h[0]) for h in hyps) == 2
    for y, _, s in hyps:
        assert abs(s - want[tuple(y)]) <= 1e-12, (y, s, want[tuple(y)])


def test_a_one_frame_utterance():
    pe, predict, joint = _table(seed=2)
    hyps, _, merges = br.rnnt_beam_ref(pe, 1, predict, joint, 4, 50)
    lp = torch.log_softmax(joint(pe[0], predict(1, None)[0]), dim=-1)
    order = sorted(range(3), key=lambda k: -float(lp[k]))
    assert merges == 0 and len(hyps) == 3                                          # slots 3 .. never became live
    assert [h[0] for h in hyps] == [[k] if k else [] for k in order]
    assert [h[1] for h in hyps] == [[0] if k else [] for k in order]
    assert [h[2] for h in hyps] == [float(lp[k]) for k in order]


def test_width_one_is_one_symbol_per_frame_argmax_and_not_greedy():
    """W = 1: at every frame the arg-max is taken and the search moves on, token or blank.  The greedy decoder at max_symbols = 1
    looks at the frame again after an emission and pays its blank there: more decisions, another score."""
    ref = rr.TransducerRef({k: v.double() for k, v in rr.transducer_weights(seed=24).items()})
    ref.sd['joint.output.weight'] = ref.sd['joint.output.weight'] * 16.0
    pe = ref.project_encoder(torch.randn((9, 64), generator=torch.Generator().manual_seed(3), dtype=torch.float64))
    for max_len in (50, 2):
        hyps, _, merges = br.rnnt_beam_ref(pe, 9, ref.predict, ref.joint_logits, 1, max_len)
        tokens, frames, score = [], [], 0.0
        pg, state = ref.predict(1, None)
        for t in range(9):
            lp = torch.log_softmax(ref.joint_logits(pe[t], pg), dim=-1)
            k = int(torch.argmax(lp)) if len(tokens) < max_len else 0
            score += float(lp[k])
            if k:
                tokens.append(k)
                frames.append(t)
                pg, state = ref.predict(k, state)
        assert merges == 0 and len(hyps) == 1
        assert hyps[0][0] == tokens and hyps[0][1] == frames and abs(hyps[0][2] - score) <= 1e-12 * abs(score)
        assert 0 < len(tokens) <= max_len
    g_tokens, _, g_score, _ = rr.rnnt_greedy_ref(pe, 9, ref.predict, ref.joint_logits, 1, 50)
    hyps, _, _ = br.rnnt_beam_ref(pe, 9, ref.predict, ref.joint_logits, 1, 50)
    assert hyps[0][2] != g_score                                                  # greedy paid blanks the beam did not


def test_the_tie_rule_on_exactly_equal_logits():
    """every candidate scores -ln 4: a stay before an extension, then the lower parent slot, then the lower token"""
    tokens = torch.tensor([[2, 0, 0], [3, 0, 0], [0, 0, 0]])
    frames = torch.zeros((3, 3), dtype=torch.int64)
    out = br.beam_step_ref(torch.zeros((3, 4), dtype=torch.float64), 1, torch.tensor([0.0, 0.0, -br.INF], dtype=torch.float64),
                           torch.tensor([1, 1, 0]), tokens, frames, 3)
    assert out['parent'] == [0, 1, 0] and out['step_tok'] == [0, 0, 1] and out['emit'] == [0, 0, 1] and out['n'] == [1, 1, 2]
    assert out['tokens'] == [[2], [3], [2, 1]] and out['frames'] == [[0], [0], [0, 1]] and out['gap'] == 0.0
    assert out['score'].tolist() == [-math.log(4.0)] * 3
    # the lower parent decides before the lower token: slot 0 offers 3, slot 1 offers 1
    lg = torch.full((2, 4), -50.0, dtype=torch.float64)
    lg[0, 3] = lg[1, 1] = 0.0
    out = br.beam_step_ref(lg, 0, torch.zeros(2, dtype=torch.float64), torch.tensor([1, 1]), tokens[:2], frames[:2], 3)
    assert out['parent'] == [0, 1] and out['step_tok'] == [3, 1] and float(out['score'][0]) == float(out['score'][1])


def test_a_merge_is_counted_and_adds_the_two_scores():
    """slot 0 holds (2), slot 1 holds (2, 1): the extension of slot 0 by 1 names slot 1's sequence and joins its stay"""
    tokens = torch.tensor([[2, 0, 0], [2, 1, 0]])
    frames = torch.tensor([[0, 0, 0], [0, 1, 0]])
    lg = torch.tensor([[0.0, 1.0, -1.0, 0.5], [0.3, -0.2, 0.1, 0.0]], dtype=torch.float64)
    sc = torch.tensor([-0.5, -1.0], dtype=torch.float64)
    out = br.beam_step_ref(lg, 2, sc, torch.tensor([1, 2]), tokens, frames, 3)
    lp = torch.log_softmax(lg, dim=-1)
    merged = float(torch.logaddexp(sc[1] + lp[1, 0], sc[0] + lp[0, 1]))
    assert out['merges'] == 1
    r = out['tokens'].index([2, 1])
    assert out['parent'][r] == 1 and out['emit'][r] == 0 and out['frames'][r] == [0, 1] and abs(float(out['score'][r]) - merged) < 1e-15
    assert out['tokens'].count([2, 1]) == 1


# ---------------------------------------------------------------------------------------------- the host side
def _refuses(fn, *args, error=ValueError, **kw):
    with pytest.raises(error) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(fn.__name__ + ': '), str(e.value)


@pytest.fixture
def no_device(monkeypatch):
    """host tensors get past the device check, and the library must not be reached"""
    monkeypatch.setattr(loss_ops, '_cuda', lambda *ts: None)
    monkeypatch.setattr(_lib, 'load', lambda *a: pytest.fail('the library was reached'))


def test_rnnt_beam_refuses_under_its_own_name(no_device):
    f32 = torch.zeros
    i32 = lambda *sh: torch.ones(sh, dtype=torch.int32)      # noqa: E731
    step = out = lambda *a: pytest.fail('the predictor was reached')      # noqa: E731
    _refuses(ops.rnnt_beam, f32(2, 8), i32(2), step, out)                                               # rank
    _refuses(ops.rnnt_beam, f32(2, 4, 6), i32(2), step, out)                                            # J % 4
    _refuses(ops.rnnt_beam, f32(2, 4, 8), f32(2), step, out)                                            # enc_len as float
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(3), step, out)                                            # B entries
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, beam_width=0)
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, beam_width=ops.RNNT_BEAM_MAX + 1)
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, beam_width=2.0)                            # an integer as float
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, max_len=0)
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, max_len=ops.RNNT_BEAM_MAX_LEN + 1)
    _refuses(ops.rnnt_beam, f32(4096, 1, 4), i32(4096), step, out, beam_width=16)                       # 65536 rows
    _refuses(ops.rnnt_beam, f32(2, 4, 8), i32(2), step, out, blank=-1)
    _refuses(ops.rnnt_beam, f32(2, 4, 8).double(), i32(2), step, out, error=_lib.OtransHipError)
    assert (ops.RNNT_BEAM_MAX, ops.RNNT_BEAM_MAX_LEN) == (16, 256)


def test_the_library_refuses_bad_beam_arguments_before_any_launch():
    """no GPU here: a refused call returns < 0 and names its entry"""
    lib = _lib.load()
    al, al2, odd = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(4096 + 4)

    def joint(B=2, W=4, T=3, t=0, J=8, pe=al, z16=None):
        return lib.otr_rnnt_beam_joint(pe, al, al, al, B, W, T, t, J, al, z16, None)
    for kw in (dict(W=17), dict(W=0), dict(B=0), dict(B=4096, W=16), dict(t=3), dict(t=-1), dict(J=6), dict(J=0), dict(pe=odd), dict(pe=None)):
        assert joint(**kw) < 0 and b'rnnt_beam_joint' in lib.otr_last_error_string(), kw

    def select(B=2, W=4, T=3, t=0, V=5, ld=5, blank=0, max_len=8, logits=al, out=al2):
        return lib.otr_rnnt_beam_select(logits, ld, al, B, W, T, t, V, blank, max_len, al, al, al, al, out, out, out, out, al, al, al, None)
    for kw in (dict(W=17), dict(W=0), dict(B=4096, W=16), dict(t=3), dict(V=1, ld=1), dict(ld=4), dict(blank=5), dict(max_len=0),
               dict(max_len=257), dict(logits=None), dict(out=al), dict(out=None)):
        assert select(**kw) < 0 and b'rnnt_beam_select' in lib.otr_last_error_string(), kw
    ptrs, other, nb = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(8192), (C.c_int32 * 1)(8)
    bad = (C.c_int32 * 1)(6)
    for args in ((al, ptrs, ptrs, nb, 1, 2, 4), (al, ptrs, other, bad, 1, 2, 4), (al, ptrs, other, nb, 17, 2, 4), (al, ptrs, other, nb, 0, 2, 4),
                 (al, ptrs, other, nb, 1, 2, 17), (None, ptrs, other, nb, 1, 2, 4)):
        assert lib.otr_rnnt_beam_gather(*args, None) < 0 and b'rnnt_beam_gather' in lib.otr_last_error_string(), args[3:]


def _model():
    import opentransformer_amd as ota
    return ota.TransducerModel(rc.model_config())


def test_the_recognizer_refuses_before_the_device_is_touched(no_device):
    import opentransformer_amd as ota
    from opentransformer_amd.recognize import build_recognizer
    model = _model()
    with pytest.raises(NotImplementedError, match="TransducerRecognizer mode 'viterbi'"):
        ota.TransducerRecognizer(model, mode='viterbi')
    with pytest.raises(ValueError, match="mbr=True needs mode='beam'"):
        ota.TransducerRecognizer(model, mbr=True)
    with pytest.raises(ValueError, match=r'nbest=5 must be in \[1, beam_width=4\]'):
        ota.TransducerRecognizer(model, mode='beam', beam_width=4, nbest=5)
    for w in (0, 17):
        with pytest.raises(ValueError, match=r'beam_width=%d must be in \[1, 16\]' % w):
            ota.TransducerRecognizer(model, mode='beam', beam_width=w)
    with pytest.raises(ValueError, match=r'max_len=300 must be in \[1, 256\]'):
        ota.TransducerRecognizer(model, mode='beam', max_len=300)
    with pytest.raises(ValueError, match='mbr_scale'):
        ota.TransducerRecognizer(model, mode='beam', mbr_scale=float('nan'))
    rec = ota.TransducerRecognizer(model, max_len=300)                              # greedy keeps its own limits
    assert (rec.mode, rec.beam_width, rec.nbest, rec.mbr, rec.max_symbols, rec.max_len) == ('greedy', 4, 1, False, 4, 300)
    # and ignores the beam's arguments: a namespace shared with the other recognizers builds the greedy recognizer it always built
    shared = types.SimpleNamespace(beam_width=20, nbest=5, max_len=300, lm_weight=0.1, ngpu=1)
    assert build_recognizer('transducer', model, None, shared, None).mode == 'greedy'
    assert ota.TransducerRecognizer(model, beam_width=0, nbest=7).mode == 'greedy'
    x = torch.zeros((1, 20, 80))
    for call in (rec.recognize_tokens_with_confidence, rec.recognize_with_confidence):
        with pytest.raises(ValueError, match="confidences need mode='beam'"):
            call(x, torch.ones((1, 20), dtype=torch.bool))


def test_the_registries_know_the_beam():
    import opentransformer_amd as ota
    from opentransformer_amd.recognize import build_recognizer
    for name, nargs in (('otr_rnnt_beam_joint', 12), ('otr_rnnt_beam_select', 22), ('otr_rnnt_beam_gather', 8)):
        assert len(_lib.SIGNATURES[name]) == nargs
    assert ops.rnnt_beam is loss_ops.rnnt_beam
    model = _model()
    units = {i: 'u%d' % i for i in range(100)}
    args = types.SimpleNamespace(max_symbols=2, max_len=17, ngpu=1, mode='beam', beam_width=6, nbest=3, mbr=True, mbr_scale=0.5)
    rec = build_recognizer('transducer', model, None, args, units)
    assert isinstance(rec, ota.TransducerRecognizer)
    assert (rec.mode, rec.beam_width, rec.nbest, rec.mbr, rec.mbr_scale, rec.max_len, rec.max_symbols) == ('beam', 6, 3, True, 0.5, 17, 2)
    rec = build_recognizer('transducer', model, None, types.SimpleNamespace(), units)      # nothing named: today's greedy recognizer
    assert (rec.mode, rec.beam_width, rec.nbest, rec.mbr, rec.mbr_scale, rec.max_len, rec.max_symbols) == ('greedy', 4, 1, False, 1.0, 200, 4)
