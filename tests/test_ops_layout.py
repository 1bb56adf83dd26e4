"""Where the wrappers live: ops.py keeps the autograd core, the switches and the shared state, decode_ops.py and data_ops.py hold the
no-autograd leaves over _runtime.py, loss_ops.py holds the losses over ops itself, and `ops` stays the one namespace callers use.
Also: every wrapper that shares a private body with a twin still signs its refusals with its own name.  No GPU, no library call."""
import os
import subprocess
import sys
import types

import pytest
import torch

from opentransformer_amd import _lib, _runtime, data_ops, decode_ops, loss_ops, ops
from opentransformer_amd.bias import PhraseBias

DECODE_NAMES = {'log_softmax', 'ctc_prefix_beam_search', 'ctc_prefix_beam_search_lm', 'ctc_prefix_beam_search_bias', 'ngram_lookup',
                'ngram_score_candidates', 'ngram_score_sequences', 'bias_score_candidates', 'bias_score_sequences', 'ctc_forced_align',
                'ctc_segment', 'edit_distance', 'edit_align', 'nbest_consensus', 'joint_prebeam', 'ctc_prefix_score', 'rescore_pack',
                'attention_rescore', 'CTC_ALIGN_MAX_TGT', 'CTC_SEGMENT_MAX_TGT', 'EDIT_MAX_LEN', 'EDIT_MAX_NBEST', 'NBEST_MAX_LEN',
                'JOINT_MAX_K', 'JOINT_MAX_T', 'JOINT_MAX_V', 'JOINT_MAX_BEAM', 'RESCORE_MAX_W', 'RESCORE_MAX_V'}
DATA_NAMES = {'feature_prepare', 'cmvn_accumulate', 'FEATPREP_MAX_RANGES', 'mixspeech_mix', 'ngram_train_count', 'ngram_train_stats',
              'ngram_train_estimate', 'NGRAM_TRAIN_ERRORS'}
LOSS_NAMES = {'LabelSmoothingLossFn', 'LabelSmoothingLossFusedFn', 'label_smoothing_loss', 'CTCLossFn', 'CTC_MAX_TGT', 'CTCLossPairFn',
              'ctc_loss_pair', 'MWER_MAX_NBEST', 'MWER_MAX_V', 'MwerLossFn', 'mwer_loss', 'DISTILL_MAX_V', 'DISTILL_MAX_K', 'DistillLossFn',
              'distill_loss', 'distill_loss_topk', 'topk_rows'}


def test_ops_is_the_namespace_of_the_leaf_modules():
    mods = (decode_ops, data_ops, loss_ops)
    for mod in mods:
        assert len(mod.__all__) == len(set(mod.__all__))
        for name in mod.__all__:
            assert getattr(ops, name) is getattr(mod, name), name
    for i, a in enumerate(mods):
        for b in mods[i + 1:]:
            assert set(a.__all__).isdisjoint(b.__all__), (a.__name__, b.__name__)
    assert set(decode_ops.__all__) == DECODE_NAMES and set(data_ops.__all__) == DATA_NAMES and set(loss_ops.__all__) == LOSS_NAMES
    assert ops._ls_ticket is loss_ops._ls_ticket                    # the one private name of the losses that a test reads through ops
    assert ops.mixspeech_mix is data_ops.mixspeech_mix              # no gradient: it went to the data leaves, not to the losses


def test_the_loss_switch_has_one_owner():
    """ops._LS_FUSED is what the tests assign and OTR_SWITCHES sets; a copy in loss_ops would make both measure the default twice"""
    assert not hasattr(loss_ops, '_LS_FUSED') and ops._LS_FUSED is True
    env = dict(os.environ, OTR_SWITCHES='ops._LS_FUSED=0')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # python -c looks in its working directory first
    out = subprocess.run([sys.executable, '-c', 'from opentransformer_amd import ops; print(ops._LS_FUSED)'], env=env, cwd=root,
                         capture_output=True, text=True, check=True)
    assert out.stdout.strip() == 'False', (out.stdout, out.stderr)


def test_ops_shares_the_runtime_objects():
    for name in ('_state', '_p', '_stream', '_cuda', '_timed', 'set_kernel_timer'):
        assert getattr(ops, name) is getattr(_runtime, name), name
    ops.set_kernel_timer(None)
    assert 'ktimer' in _runtime._state and _runtime._state is ops._state


def test_no_leaf_module_holds_ops():
    for mod in (decode_ops, data_ops, _runtime):
        held = [name for name, value in vars(mod).items() if value is ops]
        assert held == [], (mod.__name__, held)


def _starts_with_own_name(fn, *args, error=ValueError, **kw):
    with pytest.raises(error) as info:
        fn(*args, **kw)
    assert str(info.value).startswith(fn.__name__ + ': '), str(info.value)


def test_folded_wrappers_refuse_under_their_own_name_before_the_device_check():
    """one argument each that is refused on the host before any tensor's device is looked at"""
    i64 = lambda *sh: torch.zeros(sh, dtype=torch.int64)    # noqa: E731
    for fn in (ops.edit_distance, ops.edit_align):
        _starts_with_own_name(fn, i64(4), i64(1), i64(1, 2, 4))                           # 1-D ref
        _starts_with_own_name(fn, i64(1, 4), i64(1), i64(1, ops.EDIT_MAX_NBEST + 1, 4))   # the shared n-best depth check
    _starts_with_own_name(ops.edit_distance, i64(1, ops.EDIT_MAX_LEN + 1), i64(1), i64(1, 2, 4))      # each its own width limit
    _starts_with_own_name(ops.edit_align, i64(1, ops.NBEST_MAX_LEN + 1), i64(1), i64(1, 2, 4))
    with pytest.raises(_lib.OtransHipError, match='CUDA/HIP'):      # NBEST_MAX_LEN < width <= EDIT_MAX_LEN: edit_distance gets to the device
        ops.edit_distance(i64(1, ops.NBEST_MAX_LEN + 1), i64(1), i64(1, 2, 4))
    _starts_with_own_name(ops.nbest_consensus, i64(2, 4))                                 # 2-D tokens
    _starts_with_own_name(ops.nbest_consensus, i64(1, ops.EDIT_MAX_NBEST + 1, 4))
    lp, ln = torch.zeros(1, 6, 5), torch.tensor([6])
    for fn in (ops.ctc_forced_align, ops.ctc_segment):
        _starts_with_own_name(fn, lp, ln, i64(3), torch.tensor([3]))                      # 1-D targets
    _starts_with_own_name(ops.ctc_segment, lp, ln, i64(1, 0), torch.tensor([0]))          # no label column: align's case alone
    with pytest.raises(_lib.OtransHipError, match='CUDA/HIP'):
        ops.ctc_forced_align(lp, ln, i64(1, 0), torch.tensor([0]))
    tokens, out_len, scores = i64(1, 33, 4), torch.zeros(1, 33, dtype=torch.int32), torch.zeros(1, 33)
    _starts_with_own_name(ops.rescore_pack, tokens, out_len, scores, 5, 10)               # W = 33
    _starts_with_own_name(ops.attention_rescore, torch.zeros(33 * 5, 10), tokens, out_len, scores, 5, 10, 0.5)


def test_folded_wrappers_refuse_under_their_own_name_behind_the_device_check(monkeypatch):
    """the shared bodies whose first refusal of their own lies behind the device check: with that check stubbed out, host tensors
    reach it, and it is raised before the library is touched"""
    monkeypatch.setattr(decode_ops, '_cuda', lambda *ts: None)
    monkeypatch.setattr(_lib, 'load', lambda *a: pytest.fail('the library was reached'))
    err = dict(error=_lib.OtransHipError)
    i32 = lambda *sh: torch.zeros(sh, dtype=torch.int32)    # noqa: E731
    lm, pb = types.SimpleNamespace(oov_score=-10.0, vocab_size=12), PhraseBias([[2, 3]], 12)
    _starts_with_own_name(ops.ngram_score_candidates, lm, i32(2, 3), i32(2, 4), torch.zeros(2, 4), 0.5, 0.0, 1, **err)     # preds int32
    _starts_with_own_name(ops.bias_score_candidates, pb, i32(2, 3), i32(2, 4), torch.zeros(2, 4), 1, **err)
    _starts_with_own_name(ops.ngram_score_sequences, lm, i32(2, 3), i32(2), **err)                                       # tokens int32
    _starts_with_own_name(ops.bias_score_sequences, pb, i32(2, 3), i32(2), **err)
    flat, ln = torch.zeros(4, 12), torch.tensor([4])                                                                    # 2-D log_probs
    _starts_with_own_name(ops.ctc_prefix_beam_search, flat, ln, **err)
    _starts_with_own_name(ops.ctc_prefix_beam_search_lm, flat, ln, lm, 0.5, 0.0, **err)
    _starts_with_own_name(ops.ctc_prefix_beam_search_bias, flat, ln, pb, **err)
    for fn in (ops.ctc_forced_align, ops.ctc_segment):
        _starts_with_own_name(fn, flat, ln, torch.zeros(1, 3, dtype=torch.int64), torch.tensor([3]), **err)
    for fn in (ops.edit_distance, ops.edit_align):
        _starts_with_own_name(fn, torch.zeros(1, 4), ln, torch.zeros(1, 2, 4), **err)                                     # float tokens
    _starts_with_own_name(ops.nbest_consensus, torch.zeros(1, 2, 4), **err)


def test_loss_wrappers_refuse_under_their_own_name_before_the_device_check():
    """the checks that two wrappers share (_lam_check, _distill_args) and one host-side limit each of the rest"""
    i64 = lambda *sh: torch.zeros(sh, dtype=torch.int64)    # noqa: E731
    ln = i64(2)
    for lam in (torch.zeros(2), 0.5):                                                     # two elements; a Python float
        _starts_with_own_name(ops.ctc_loss_pair, torch.zeros(2, 6, 5), i64(2, 3), i64(2, 3), ln, ln, ln, lam)
        _starts_with_own_name(ops.mixspeech_mix, torch.zeros(4, 6, 5), i64(4), lam)
    _starts_with_own_name(ops.distill_loss, torch.zeros(2, 6, 5), torch.zeros(2, 6, 5), ln, temperature=0)
    _starts_with_own_name(ops.distill_loss_topk, torch.zeros(2, 6, 5), torch.zeros(2, 6, 4), torch.zeros(2, 6, 4, dtype=torch.int32), ln,
                          temperature=0)
    N = ops.MWER_MAX_NBEST + 1
    _starts_with_own_name(ops.mwer_loss, torch.zeros(N, 3, 5), i64(N, 3), torch.zeros(N, dtype=torch.int32),
                          torch.zeros(1, N, dtype=torch.int32))
    _starts_with_own_name(ops.topk_rows, torch.zeros(2, 6, 5), ln, 0)


def test_loss_wrappers_refuse_under_their_own_name_behind_the_device_check(monkeypatch):
    """the dtype refusals, which lie behind the device check: every integer argument sent as float32"""
    for mod in (loss_ops, data_ops):
        monkeypatch.setattr(mod, '_cuda', lambda *ts: None)
    monkeypatch.setattr(_lib, 'load', lambda *a: pytest.fail('the library was reached'))
    err = dict(error=_lib.OtransHipError)
    f32, lam = torch.zeros, torch.zeros(1)
    _starts_with_own_name(ops.ctc_loss_pair, f32(2, 6, 5), f32(2, 3), f32(2, 3), f32(2), f32(2), f32(2), lam, **err)
    _starts_with_own_name(ops.mixspeech_mix, f32(4, 6, 5), f32(4), lam, **err)
    _starts_with_own_name(ops.distill_loss_topk, f32(2, 6, 5), f32(2, 6, 4), f32(2, 6, 4), f32(2), **err)
    _starts_with_own_name(ops.mwer_loss, f32(4, 3, 5), f32(4, 3), f32(4), f32(2, 2), **err)
