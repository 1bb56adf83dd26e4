"""CPU (-m "not gpu"): minimum word error rate training.  The numpy float64 restatement (tests/mwer_ref.py) has the properties the loss
promises, and the library's entry points and ops.mwer_loss refuse what is outside the documented limits before they launch."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from tests import mwer_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def _live_elements(rng, ys_out, n_rows, errors, V, count):
    """(h, l, v) inside the rows of slots that can carry a gradient, the target column among them"""
    N = errors.shape[1]
    hs = [h for h in range(len(n_rows)) if n_rows[h] > 0 and errors[h // N, h % N] >= 0]
    picks = []
    for _ in range(count):
        h = hs[rng.integers(len(hs))]
        l = int(rng.integers(n_rows[h]))
        picks.append((h, l, int(ys_out[h, l]) if rng.random() < 0.3 else int(rng.integers(V))))
    return picks


@pytest.mark.parametrize('N', [2, 5])
def test_restatement_matches_its_finite_differences(N):
    rng = np.random.default_rng(N)
    B, max_len, V = 4, 9, 23
    x, ys_out, n_rows, errors = ref.case(rng, B, N, max_len, V)
    errors[1, 0] = -1                                         # an invalid pair: left out of the softmax
    f = ref.forward(x, ys_out, n_rows, errors, V)
    assert f['b_live'] == B and not f['live'][1, 0] and np.abs(f['c']).max() > 1e-3
    picks = _live_elements(rng, ys_out, n_rows, errors, V, 60)
    assert ref.finite_difference_error(x, ys_out, n_rows, errors, V, picks) < 1e-8
    d = ref.grad(x, ys_out, n_rows, errors, V)
    assert not d[1 * N + 0].any()                             # the invalid slot has no gradient
    for h in range(B * N):
        assert not d[h, n_rows[h]:].any()                     # nor have rows at or past n_rows


def test_one_hypothesis_or_equal_errors_give_the_errors_and_no_gradient():
    rng = np.random.default_rng(0)
    V = 17
    x, ys_out, n_rows, errors = ref.case(rng, 3, 1, 7, V)
    f = ref.forward(x, ys_out, n_rows, errors, V)
    assert f['loss'] == errors.mean() and not ref.grad(x, ys_out, n_rows, errors, V).any()
    x, ys_out, n_rows, errors = ref.case(rng, 3, 4, 7, V)
    errors[:] = 3
    f = ref.forward(x, ys_out, n_rows, errors, V)
    assert abs(f['loss'] - 3.0) < 1e-12 and np.abs(ref.grad(x, ys_out, n_rows, errors, V)).max() < 1e-15
    assert np.abs(f['c']).max() < 1e-15                        # P (W - E) vanishes: the centring term


def test_dead_utterances_and_bad_targets():
    rng = np.random.default_rng(1)
    B, N, max_len, V = 3, 3, 6, 11
    x, ys_out, n_rows, errors = ref.case(rng, B, N, max_len, V)
    base = ref.forward(x, ys_out, n_rows, errors, V)
    assert base['b_live'] == 3
    # an utterance with no live slot adds nothing and is not counted
    n2 = n_rows.copy()
    n2[N:2 * N] = 0
    f = ref.forward(x, ys_out, n2, errors, V)
    assert f['b_live'] == 2 and f['utt_err'][1] == 0 and not f['post'][1].any()
    assert abs(f['loss'] - (base['utt_err'][0] + base['utt_err'][2]) / 2) < 1e-12
    assert not ref.grad(x, ys_out, n2, errors, V)[N:2 * N].any()
    # no live slot anywhere: loss 0, gradient 0
    f = ref.forward(x, ys_out, np.zeros_like(n_rows), errors, V)
    assert f['b_live'] == 0 and f['loss'] == 0.0 and not ref.grad(x, ys_out, np.zeros_like(n_rows), errors, V).any()
    # a target outside [0, V) kills its slot (and only it)
    for bad in (V, -1, 1 << 40):
        y2 = ys_out.copy()
        y2[0, 0] = bad
        f = ref.forward(x, y2, n_rows, errors, V)
        assert not f['live'][0, 0] and f['live'][0, 1:].all() and f['seq_logp'][0, 0] == -np.inf and f['post'][0, 0] == 0
        assert abs(f['post'][0].sum() - 1) < 1e-12 and not ref.grad(x, y2, n_rows, errors, V)[0].any()


@pytest.mark.parametrize('eta', [0.1, 1.0])
def test_a_gradient_step_lowers_the_expected_errors(eta):
    rng = np.random.default_rng(2)
    V = 29
    x, ys_out, n_rows, errors = ref.case(rng, 4, 4, 9, V)
    g = ref.grad(x, ys_out, n_rows, errors, V)
    before = ref.forward(x, ys_out, n_rows, errors, V)['loss']
    after = ref.forward(x - eta * g, ys_out, n_rows, errors, V)['loss']
    assert np.abs(g).max() > 1e-4 and after < before, (before, after)


def test_abi_version_is_608_everywhere():
    header = (ROOT / 'include' / 'otrans_hip.h').read_text()
    assert re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1) == '608'
    assert '608: otr_mwer_workspace_floats and otr_mwer_loss' in header
    assert _lib.OTR_ABI_VERSION == 608
    for kind in ('bf16', 'fp16'):
        assert _lib.load(kind).otr_version() == 608
    assert 'otr_mwer_loss' in _lib.SIGNATURES and 'otr_mwer_workspace_floats' in _lib.SIGNATURES


def test_workspace_size_and_bad_shapes():
    lib = _lib.load()
    assert lib.otr_mwer_workspace_floats(32, 4, 32) == 32 * 4 * 32 + 32 * 4
    assert lib.otr_mwer_workspace_floats(0, 4, 32) == 0
    for B, N, max_len in ((4, 0, 9), (4, 33, 9), (4, 4, 0), (-1, 4, 9), (1 << 20, 32, 32)):
        assert lib.otr_mwer_workspace_floats(B, N, max_len) == -1, (B, N, max_len)


def test_entry_point_refuses_bad_arguments_and_leaves_the_outputs_alone():
    """checked on the host before any launch (no GPU needed): every output buffer still holds its fill afterwards"""
    lib = _lib.load()
    fill = 123.25
    bufs = {k: (C.c_float * 64)(*([fill] * 64)) for k in ('loss', 'seq', 'post', 'utt', 'dl', 'ws')}
    p = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}
    inp = C.cast((C.c_float * 64)(), C.c_void_p)

    def call(logits=inp, ld=100, ys=inp, ld_ys=9, n_rows=inp, errors=inp, B=2, N=4, max_len=9, V=100, loss=p['loss'], seq=p['seq'],
             post=p['post'], utt=p['utt'], dl=p['dl'], ldd=100, ws=p['ws'], nws=1 << 20):
        return lib.otr_mwer_loss(logits, ld, ys, ld_ys, n_rows, errors, B, N, max_len, V, None, loss, seq, post, utt, dl, ldd, ws, nws, None)
    bad = [dict(logits=None), dict(ys=None), dict(n_rows=None), dict(errors=None), dict(loss=None), dict(seq=None), dict(post=None),
           dict(utt=None), dict(N=0), dict(N=33), dict(V=0), dict(V=8193, ld=8200, ldd=8200), dict(ld=99), dict(ldd=99), dict(ld_ys=8),
           dict(max_len=0), dict(B=-1), dict(B=1 << 20, N=32, max_len=32), dict(ws=None), dict(nws=2 * 4 * 9 + 2 * 4 - 1)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b'mwer_loss' in lib.otr_last_error_string(), kw
    for k, b in bufs.items():
        assert all(v == fill for v in b), k
    assert call(B=0) == 0                                      # nothing to do: no launch
    assert all(v == fill for v in bufs['loss'])


def test_ops_refuse_before_they_look_at_the_device():
    from opentransformer_amd import ops
    assert ops.MWER_MAX_NBEST == 32
    B, N, max_len, V = 2, 3, 5, 10
    lg = torch.zeros(B * N, max_len, V)
    ys = torch.zeros((B * N, max_len), dtype=torch.long)
    nr, er = torch.ones(B * N, dtype=torch.int32), torch.zeros((B, N), dtype=torch.int32)
    with pytest.raises(_lib.OtransHipError):                   # CPU tensors: there is no fallback
        ops.mwer_loss(lg, ys, nr, er)
    with pytest.raises(ValueError, match='N=33'):
        ops.mwer_loss(torch.zeros(33, max_len, V), torch.zeros((33, max_len), dtype=torch.long), torch.ones(33, dtype=torch.int32),
                      torch.zeros((1, 33), dtype=torch.int32))
    with pytest.raises(ValueError, match='V=9000'):
        ops.mwer_loss(torch.zeros(B * N, max_len, 9000), ys, nr, er)
    with pytest.raises(ValueError, match='rows'):
        ops.mwer_loss(lg[:-1], ys, nr, er)
    with pytest.raises(ValueError, match='errors'):
        ops.mwer_loss(lg, ys, nr, er.view(-1))
