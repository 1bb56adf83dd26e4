"""Where the wrappers live: ops.py keeps the autograd code and the shared state, decode_ops.py and data_ops.py hold the no-autograd
leaves over _runtime.py, and `ops` stays the one namespace callers use.  Also: every wrapper that shares a private body with a twin
still signs its refusals with its own name.  No GPU, no library call."""
import types

import pytest
import torch

from opentransformer_amd import _lib, _runtime, data_ops, decode_ops, ops
from opentransformer_amd.bias import PhraseBias

DECODE_NAMES = {'log_softmax', 'ctc_prefix_beam_search', 'ctc_prefix_beam_search_lm', 'ctc_prefix_beam_search_bias', 'ngram_lookup',
                'ngram_score_candidates', 'ngram_score_sequences', 'bias_score_candidates', 'bias_score_sequences', 'ctc_forced_align',
                'ctc_segment', 'edit_distance', 'edit_align', 'nbest_consensus', 'joint_prebeam', 'ctc_prefix_score', 'rescore_pack',
                'attention_rescore', 'CTC_ALIGN_MAX_TGT', 'CTC_SEGMENT_MAX_TGT', 'EDIT_MAX_LEN', 'EDIT_MAX_NBEST', 'NBEST_MAX_LEN',
                'JOINT_MAX_K', 'JOINT_MAX_T', 'JOINT_MAX_V', 'JOINT_MAX_BEAM', 'RESCORE_MAX_W', 'RESCORE_MAX_V'}
DATA_NAMES = {'feature_prepare', 'cmvn_accumulate', 'FEATPREP_MAX_RANGES', 'ngram_train_count', 'ngram_train_stats',
              'ngram_train_estimate', 'NGRAM_TRAIN_ERRORS'}


def test_ops_is_the_namespace_of_the_leaf_modules():
    for mod in (decode_ops, data_ops):
        assert len(mod.__all__) == len(set(mod.__all__))
        for name in mod.__all__:
            assert getattr(ops, name) is getattr(mod, name), name
    assert set(decode_ops.__all__).isdisjoint(data_ops.__all__)
    assert set(decode_ops.__all__) == DECODE_NAMES and set(data_ops.__all__) == DATA_NAMES


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
