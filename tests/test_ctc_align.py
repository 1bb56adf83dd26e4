"""CPU (-m "not gpu"): CTC forced alignment.  The numpy restatement (tests/ctc_align_ref.py) finds the best of all paths that collapse
to the labels (brute force over every path) and keeps the documented tie rule; the library's entry points refuse bad arguments before
they launch (no GPU here); the op and the models refuse what they cannot serve."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from tests import ctc_align_ref as ref

UNIFORM_TIE_LABELS = [1, 1, 2]
# uniform log-probs, T = 7, labels [1, 1, 2]: every path scores the same, so the tie rule alone picks the path.  Traced back from the
# end: the final blank wins the last tie, and at every frame the state stays while staying is possible, i.e. each state is entered at
# the earliest frame at which it can be reached (blank, 1, blank, 1, 2 at frames 0 .. 4) and the final blank holds the rest.
UNIFORM_TIE_FRAME_TOKEN = [1, 0, 1, 2, 0, 0, 0]


def collapse(path, blank=0):
    out, last = [], None
    for c in path:
        if c != last and c != blank:
            out.append(c)
        last = c
    return out


def test_restatement_finds_the_best_of_all_paths():
    """V = 3 (blank + 2 tokens), every T <= 6 and every label sequence of L <= 3 (repeats included): all V^T paths enumerated"""
    rng = np.random.default_rng(0)
    V = 3
    for T in range(1, 7):
        lp = rng.normal(size=(T, V)) * 2.0
        lp = (lp - np.log(np.exp(lp).sum(-1, keepdims=True))).astype(np.float32)
        by_labels = {}
        for path in itertools.product(range(V), repeat=T):
            sc = float(sum(np.float64(lp[t, c]) for t, c in enumerate(path)))
            by_labels.setdefault(tuple(collapse(path)), []).append((sc, path))
        for L in range(4):
            for labels in itertools.product([1, 2], repeat=L):
                ft, spans, llp, score = ref.align(lp[None], [T], np.array([list(labels) + [0] * (3 - L)]), [L])
                paths = by_labels.get(labels)
                if not paths:
                    assert score[0] == -np.inf and (ft == -1).all() and (spans == -1).all() and (llp == 0).all(), (T, labels)
                    continue
                best = max(sc for sc, _ in paths)
                assert abs(float(score[0]) - best) <= 1e-5, (T, labels, score[0], best)
                got = tuple(ft[0].tolist())
                assert collapse(got) == list(labels)
                assert any(p == got and sc >= best - 1e-5 for sc, p in paths), (T, labels, got)      # one of the maximisers
                for j in range(L):                                               # spans and sums describe that path
                    a, e = spans[0, j]
                    assert 0 <= a < e <= T and all(got[t] == labels[j] for t in range(a, e))
                    assert abs(float(llp[0, j]) - float(sum(np.float64(lp[t, labels[j]]) for t in range(a, e)))) <= 1e-5
                assert (spans[0, L:] == -1).all() and (llp[0, L:] == 0).all()


def test_restatement_tie_rule():
    lp = np.full((1, 7, 3), np.log(1.0 / 3.0), np.float32)
    ft, spans, llp, score = ref.align(lp, [7], np.array([UNIFORM_TIE_LABELS]), [3])
    assert ft[0].tolist() == UNIFORM_TIE_FRAME_TOKEN
    assert spans[0].tolist() == [[0, 1], [2, 3], [3, 4]]
    want = np.float32(0.0)
    for _ in range(7):
        want = np.float32(want + lp[0, 0, 0])
    assert score[0] == want and (llp[0] == lp[0, 0, 0]).all()
    # no frames: the empty path for no labels, nothing for some
    ft, spans, llp, score = ref.align(lp, [0, ], np.zeros((1, 2), np.int64), [0])
    assert score[0] == 0.0 and (ft == -1).all() and (spans == -1).all()
    assert ref.align(lp, [0], np.array([[1, 2]]), [2])[3][0] == -np.inf
    assert ref.align(lp, [3], np.array([UNIFORM_TIE_LABELS]), [3])[3][0] == -np.inf          # 3 labels + 1 repeat need 4 frames
    assert ref.align(lp, [4], np.array([UNIFORM_TIE_LABELS]), [3])[0][0, :4].tolist() == [1, 0, 1, 2]
    assert ref.align(lp, [7], np.array([UNIFORM_TIE_LABELS]), [4])[3][0] == -np.inf          # a length beyond max_tgt


def test_ctc_align_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    al = C.c_void_p(4096)
    B, T, V, M = 2, 2000, 100, 20
    ws = lib.otr_ctc_align_workspace_bytes(B, T, M)
    assert ws >= B * T * 64 and ws % 8 == 0                          # past the LDS route: 64 B of back-pointers per frame
    small = lib.otr_ctc_align_workspace_bytes(B, 64, M)
    assert small > 0 and small % 8 == 0
    assert lib.otr_ctc_align_workspace_bytes(B, T, 127) > 0 and lib.otr_ctc_align_workspace_bytes(B, T, 0) > 0
    assert lib.otr_ctc_align_workspace_bytes(0, T, M) == -1 and lib.otr_ctc_align_workspace_bytes(B, 0, M) == -1
    assert lib.otr_ctc_align_workspace_bytes(B, T, 128) == -1 and lib.otr_ctc_align_workspace_bytes(B, T, -1) == -1

    def call(lp=al, ld=V, tg=al, il=al, tl=al, V=V, max_tgt=M, blank=0, workspace=al, ws_bytes=ws, ft=al, sp=al, ll=al, sc=al):
        return lib.otr_ctc_align(lp, ld, tg, max(max_tgt, 1), il, tl, B, T, V, max_tgt, blank, workspace, ws_bytes, ft, sp, ll, sc, None)
    for name in ('lp', 'tg', 'il', 'tl', 'workspace', 'ft', 'sp', 'll', 'sc'):
        assert call(**{name: None}) < 0, name
        assert b'ctc_align' in lib.otr_last_error_string() and b'null' in lib.otr_last_error_string()
    assert call(max_tgt=128) < 0 and b'127' in lib.otr_last_error_string()
    assert call(blank=V) < 0 and call(blank=-1) < 0 and b'ctc_align' in lib.otr_last_error_string()
    assert call(ld=V - 1) < 0
    assert call(V=1, ld=1) < 0
    assert call(ws_bytes=ws - 1) < 0 and b'workspace' in lib.otr_last_error_string()
    assert call(workspace=C.c_void_p(4096 + 4)) < 0 and b'aligned' in lib.otr_last_error_string()
    assert b'ctc_align' in lib.otr_last_error_string()


def test_op_refuses_cpu_tensors_and_128_label_columns():
    from opentransformer_amd import ops
    lp, il = torch.zeros(1, 4, 5), torch.tensor([4])
    with pytest.raises(_lib.OtransHipError):
        ops.ctc_forced_align(lp, il, torch.ones(1, 2, dtype=torch.long), torch.tensor([2]))
    with pytest.raises(ValueError, match='127'):
        ops.ctc_forced_align(lp, il, torch.ones(1, 128, dtype=torch.long), torch.tensor([2]))


def test_speech_to_text_align_needs_the_ctc_head():
    import opentransformer_amd as ota
    from opentransformer_amd import synthetic as syn
    model = ota.SpeechToText(syn.c1_model(ctc_weight=0.0))
    with pytest.raises(ValueError, match='ctc_weight > 0'):
        model.align(torch.zeros(1, 40, 80), torch.ones(1, 40, dtype=torch.bool), torch.ones(1, 2, dtype=torch.long), torch.tensor([2]))


def test_frames_to_seconds():
    from opentransformer_amd.recognize import frames_to_seconds
    assert frames_to_seconds(0) == 0.0 and frames_to_seconds(25) == 1.0 and frames_to_seconds(3, subsample=2, frame_shift_ms=12.5) == 0.075
