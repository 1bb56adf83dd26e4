"""CPU (-m "not gpu"): the transducer's float64 restatement (tests/rnnt_ref.py) agrees with itself -- the autograd gradient of the
diagonal sweep equals the closed form the kernel implements, on every case of tests/rnnt_cases.py -- and the host side of the
feature: the wrappers' refusals, the model's state_dict keys, the registries."""
import types

import pytest
import torch

from opentransformer_amd import _lib, loss_ops, ops
from tests import rnnt_cases as rc
from tests import rnnt_ref as rr


@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_autograd_of_the_restatement_equals_the_closed_form(name):
    c = rc.build(name)
    loss, nll, valid, g = rc.reference_of(name)
    x = c['logits'].double()
    closed, occ = rc.closed_form_of(name)
    rows = rc.rowsum_rel(g, occ)
    B = x.shape[0]
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(nll).all())
    for b in range(B):
        Tb, Ub = int(c['enc_len'][b]), int(c['tgt_len'][b])
        if not bool(valid[b]):
            assert float(nll[b]) == 0.0 and float(g[b].abs().max()) == 0.0 and float(closed[b].abs().max()) == 0.0, (name, b)
            continue
        d = float((g[b] - closed[b]).norm() / closed[b].norm())
        assert d <= 1e-12, (name, b, d)
        live = g[b, :Tb, :Ub + 1]
        assert float(rows[b].max()) <= 1e-12, (name, b)                          # every live row sums to zero (rowsum_rel says of what)
        assert float(rc.rowsum_rel(closed, occ)[b].max()) <= 1e-12, (name, b)
        assert float(live.abs().sum(-1).min()) > 0, (name, b)
        dead = g[b].clone()
        dead[:Tb, :Ub + 1] = 0
        assert float(dead.abs().max()) == 0.0, (name, b)
    if name == 'guarded':
        assert [b for b in range(B) if not bool(valid[b])] == list(rc.GUARDED_DEAD)
    assert abs(float(loss) - float(nll.sum()) / B) <= 1e-12 * abs(float(loss))


@pytest.mark.parametrize('name', ['tiny', 'ragged', 'peaked', 'vocab_65'])
def test_alpha_final_equals_beta_origin(name):
    c = rc.build(name)
    _, nll, valid, _ = rc.reference_of(name)
    for b in range(c['logits'].shape[0]):
        if not bool(valid[b]):
            continue
        Tb, Ub = int(c['enc_len'][b]), int(c['tgt_len'][b])
        alpha, beta, lp = rr.rnnt_lattice_ref(c['logits'][b].double(), c['labels'][b, :Ub], Tb, Ub)
        a = float(alpha[Tb - 1, Ub] + lp[Tb - 1, Ub, rr.BLANK])
        assert abs(a - float(beta[0, 0])) <= 1e-12 * abs(a), (name, b)
        assert abs(a + float(nll[b])) <= 1e-12 * abs(a), (name, b)              # and the diagonal sweep finds the same number


def _refuses(fn, *args, error=ValueError, **kw):
    with pytest.raises(error) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(fn.__name__ + ': '), str(e.value)


@pytest.fixture
def no_device(monkeypatch):
    """host tensors get past the device check, and the library must not be reached"""
    monkeypatch.setattr(loss_ops, '_cuda', lambda *ts: None)
    monkeypatch.setattr(_lib, 'load', lambda *a: pytest.fail('the library was reached'))


def test_rnnt_loss_refuses_under_its_own_name(no_device):
    f32 = torch.zeros
    i32 = lambda *sh: torch.ones(sh, dtype=torch.int32)      # noqa: E731
    i64 = lambda *sh: torch.ones(sh, dtype=torch.int64)      # noqa: E731
    _refuses(ops.rnnt_loss, f32(2, 3, 5), i32(2), i64(2, 2), i32(2))                                    # rank
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(2), i64(2), i32(2))                                    # labels' rank
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(2), i64(2, 1), i32(2))                                 # labels narrower than U
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), f32(2), i64(2, 2), i32(2))                                 # enc_len as float
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(2), i64(2, 2), f32(2))                                 # tgt_len as float
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(2), f32(2, 2), i32(2))                                 # labels as float
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(3), i64(2, 2), i32(2))                                 # B entries
    _refuses(ops.rnnt_loss, f32(1, 1, ops.RNNT_MAX_TGT + 2, 3), i32(1), i64(1, ops.RNNT_MAX_TGT + 1), i32(1))    # too many columns
    _refuses(ops.rnnt_loss, f32(2, 3, 3, 5), i32(2), i64(2, 2), i32(2), blank=5)
    _refuses(ops.rnnt_loss, torch.zeros(2, 3, 3, 5, dtype=torch.float64), i32(2), i64(2, 2), i32(2), error=_lib.OtransHipError)


def test_rnnt_joint_refuses_under_its_own_name(no_device):
    f32 = torch.zeros
    i32 = lambda *sh: torch.ones(sh, dtype=torch.int32)      # noqa: E731
    _refuses(ops.rnnt_joint, f32(2, 8), f32(2, 3, 8), i32(2), i32(2))                                   # rank
    _refuses(ops.rnnt_joint, f32(2, 4, 8), f32(2, 3, 12), i32(2), i32(2))                               # J differs
    _refuses(ops.rnnt_joint, f32(2, 4, 6), f32(2, 3, 6), i32(2), i32(2))                                # J % 4
    _refuses(ops.rnnt_joint, f32(1, 2, 4), f32(1, ops.RNNT_MAX_TGT + 2, 4), i32(1), i32(1))             # too many columns
    _refuses(ops.rnnt_joint, f32(2, 4, 8), f32(2, 3, 8), f32(2), i32(2))                                # enc_len as float
    _refuses(ops.rnnt_joint, f32(2, 4, 8), f32(2, 3, 8), i32(2), f32(2))                                # tgt_len as float
    _refuses(ops.rnnt_joint, f32(2, 4, 8).double(), f32(2, 3, 8), i32(2), i32(2), error=_lib.OtransHipError)


def test_rnnt_greedy_refuses_under_its_own_name(no_device):
    f32 = torch.zeros
    i32 = lambda *sh: torch.ones(sh, dtype=torch.int32)      # noqa: E731
    step = out = lambda *a: pytest.fail('the predictor was reached')      # noqa: E731
    _refuses(ops.rnnt_greedy, f32(2, 8), i32(2), step, out)                                             # rank
    _refuses(ops.rnnt_greedy, f32(2, 4, 6), i32(2), step, out)                                          # J % 4
    _refuses(ops.rnnt_greedy, f32(2, 4, 8), f32(2), step, out)                                          # enc_len as float
    _refuses(ops.rnnt_greedy, f32(2, 4, 8), i32(2), step, out, max_symbols=1.0)                         # an integer as float
    _refuses(ops.rnnt_greedy, f32(2, 4, 8), i32(2), step, out, max_len=0)
    _refuses(ops.rnnt_greedy, f32(2, 4, 8).double(), i32(2), step, out, error=_lib.OtransHipError)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """no GPU here: a refused call returns < 0 and names its entry"""
    import ctypes as C
    lib = _lib.load()
    al, odd = C.c_void_p(4096), C.c_void_p(4096 + 4)

    def loss(B=2, T=3, U1=3, V=5, ld=5, ldl=2, blank=0, ldd=5, ws=al, nws=5 * 18 + 4, logits=al, dl=al):
        return lib.otr_rnnt_loss(logits, ld, al, ldl, al, al, B, T, U1, V, blank, None, al, al, al, dl, ldd, ws, nws, None)
    for kw in (dict(U1=257), dict(B=0), dict(T=0), dict(V=1, ld=1, ldd=1), dict(ld=4), dict(ldl=1), dict(blank=5),
               dict(ldd=4), dict(ws=None), dict(nws=5 * 18 + 3), dict(logits=None), dict(B=65535, T=65535, U1=4)):
        assert loss(**kw) < 0 and b'rnnt_loss' in lib.otr_last_error_string(), kw
    assert lib.otr_rnnt_workspace_floats(2, 3, 3) == 5 * 18 + 4 and lib.otr_rnnt_workspace_floats(2, 3, 257) == -1
    assert lib.otr_rnnt_joint_fwd(al, al, al, al, 2, 3, 3, 6, al, None, None) < 0 and b'rnnt_joint_fwd' in lib.otr_last_error_string()
    assert lib.otr_rnnt_joint_fwd(odd, al, al, al, 2, 3, 3, 8, al, None, None) < 0
    assert lib.otr_rnnt_joint_fwd(al, al, al, al, 2, 3, 257, 8, al, None, None) < 0
    assert lib.otr_rnnt_joint_bwd(al, al, al, al, 2, 3, 3, 6, al, al, None) < 0 and b'rnnt_joint_bwd' in lib.otr_last_error_string()
    assert lib.otr_rnnt_joint_bwd(al, al, al, al, 2, 3, 3, 8, al, None, None) < 0
    assert lib.otr_rnnt_greedy_joint(al, al, al, al, al, 2, 3, 6, 4, al, None, None) < 0 and b'rnnt_greedy_joint' in lib.otr_last_error_string()
    assert lib.otr_rnnt_greedy_advance(al, 4, al, 2, 3, 5, 0, 1, 4, al, al, al, al, al, al, al, al, al, None) < 0          # ld < V
    assert b'rnnt_greedy_advance' in lib.otr_last_error_string()
    assert lib.otr_rnnt_greedy_advance(al, 5, al, 2, 3, 5, 0, 0, 4, al, al, al, al, al, al, al, al, al, None) < 0          # max_symbols 0
    ptrs, same, nb = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(4096), (C.c_int32 * 1)(6)
    assert lib.otr_rnnt_greedy_commit(al, ptrs, same, nb, 1, 2, None) < 0 and b'rnnt_greedy_commit' in lib.otr_last_error_string()
    assert lib.otr_rnnt_greedy_commit(al, ptrs, same, nb, 17, 2, None) < 0


EXPECTED_KEYS = ['predictor.embedding.weight'] + ['predictor.rnn.%s_l%d' % (n, k) for k in (0, 1) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')] \
    + ['joint.enc_proj.weight', 'joint.enc_proj.bias', 'joint.pred_proj.weight', 'joint.output.weight', 'joint.output.bias']


def test_transducer_model_state_dict_keys():
    import opentransformer_amd as ota
    model = ota.TransducerModel(rc.model_config())
    keys = list(model.state_dict())
    own = [k for k in keys if k.startswith(('predictor.', 'joint.'))]
    assert sorted(own) == sorted(EXPECTED_KEYS)
    assert all(k.startswith(('frontend.', 'encoder.', 'predictor.', 'joint.')) for k in keys)
    sd = model.state_dict()
    assert tuple(sd['joint.enc_proj.weight'].shape) == (64, 64) and tuple(sd['joint.output.weight'].shape) == (100, 64)
    assert tuple(sd['predictor.rnn.weight_ih_l0'].shape) == (256, 64) and tuple(sd['predictor.embedding.weight'].shape) == (100, 64)


def test_transducer_is_registered():
    import opentransformer_amd as ota
    assert ota.End2EndModel['transducer'] is ota.TransducerModel


def test_build_recognizer_builds_the_transducer_recognizer(tmp_path):
    import opentransformer_amd as ota
    from opentransformer_amd.recognize import build_recognizer
    model = ota.TransducerModel(rc.model_config())
    args = types.SimpleNamespace(max_symbols=2, max_len=17, ngpu=1)
    rec = build_recognizer('transducer', model, None, args, {i: 'u%d' % i for i in range(100)})
    assert isinstance(rec, ota.TransducerRecognizer) and (rec.max_symbols, rec.max_len) == (2, 17)
    assert rec.model is model and not model.training
    # the checkpoint round trip keeps the four parts
    path = str(tmp_path / 'm.pt')
    model.save_checkpoint(rc.model_config(), path)
    chk = torch.load(path)
    assert sorted(chk) == ['encoder', 'frontend', 'joint', 'params', 'predictor']
    other = ota.TransducerModel(rc.model_config())
    other.load_model(chk)
    for (k, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(TypeError):
        ota.TransducerRecognizer(torch.nn.Linear(2, 2))
