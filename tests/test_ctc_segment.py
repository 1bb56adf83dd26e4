"""CPU (-m "not gpu"): CTC segmentation.  The numpy restatement (tests/ctc_segment_ref.py) equals the forced-alignment restatement with
both ends fixed, finds the best of all partial paths (brute force), recovers planted paths and keeps the documented tie rules; the
library's entry points refuse bad arguments before they launch (no GPU here) and leave the outputs alone; window_plan covers every
encoder frame once; the op refuses what it cannot serve."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from tests import ctc_align_ref
from tests import ctc_segment_ref as ref
from tests.test_ctc_align import UNIFORM_TIE_FRAME_TOKEN, UNIFORM_TIE_LABELS, collapse

LN_HALF = math.log(0.5)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'otrans_hip.h')


def log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def planted_case(rng, V=8, min_edge_span=1):
    """A CTC path planted in noise: on the planted frames the planted token has 0.9 and the others share 0.1; 0-19 uniform frames in
    front and behind.  Returns (lp [T, V], labels, front, planted tokens per planted frame)."""
    L = int(rng.integers(1, 8))
    labels = rng.integers(1, V, size=L).tolist()
    tokens = []
    for j, c in enumerate(labels):
        if j and (labels[j - 1] == c or rng.random() < 0.5):
            tokens += [0] * int(rng.integers(1, 3))                         # a blank run (needed between repeats)
        edge = j == 0 or j == L - 1
        tokens += [c] * int(rng.integers(min_edge_span if edge else 1, min_edge_span + 4 if edge else 5))
    front, behind = int(rng.integers(0, 20)), int(rng.integers(0, 20))
    p = np.full((front + len(tokens) + behind, V), 1.0 / V)
    for t, c in enumerate(tokens):
        p[front + t] = 0.1 / (V - 1)
        p[front + t, c] = 0.9
    return np.log(p).astype(np.float32), labels, front, tokens


def test_fixed_ends_equal_the_forced_alignment_restatement():
    rng = np.random.default_rng(0)
    for case in range(200):
        V = int(rng.integers(3, 12))
        L = int(rng.choice([1, 2, 3, 5, 9, 20, 127])) if case % 10 else 127
        labels = rng.integers(1, V, size=L)
        labels[rng.random(L) < 0.2] = 1                                     # adjacent repeats here and there
        need = L + int((labels[1:] == labels[:-1]).sum())
        T = need + int(rng.integers(0, 12)) - (1 if case % 7 == 0 else 0)   # some one frame short: infeasible in both
        if T < 1:
            continue
        lp = log_softmax(rng.normal(size=(1, T, V)) * 3.0)
        got = ref.segment(lp, [T], labels[None], [L], free_start=False, free_end=False, skip_logp=LN_HALF)
        want = ctc_align_ref.align(lp, [T], labels[None], [L])
        for g, w in zip(got[:4], want):
            np.testing.assert_array_equal(g, w, err_msg='case %d' % case)
        assert got[4][0].tolist() == ([0, T] if np.isfinite(want[3][0]) else [-1, -1])


def test_restatement_finds_the_best_of_all_partial_paths():
    """V = 3, T <= 5, every label sequence of 1 <= L <= 2: every stretch [a, e) of frames and every path on it enumerated; a frame
    outside the stretch costs skip_logp"""
    rng = np.random.default_rng(1)
    V = 3
    for T, skip in itertools.product(range(1, 6), (0.0, LN_HALF, -3.0)):
        lp = log_softmax(rng.normal(size=(T, V)) * 2.0)
        for fs, fe in itertools.product((False, True), repeat=2):
            best = {}
            for a in range(0, T if fs else 1):
                for e in range(a + 1 if fe else T, T + 1):
                    for path in itertools.product(range(V), repeat=e - a):
                        sc = float(sum(np.float64(lp[a + t, c]) for t, c in enumerate(path))) + skip * (T - (e - a))
                        key = tuple(collapse(path))
                        best[key] = max(best.get(key, -np.inf), sc)
            for L in (1, 2):
                for labels in itertools.product([1, 2], repeat=L):
                    ft, spans, llp, score, bounds = ref.segment(lp[None], [T], np.array([list(labels)]), [L], free_start=fs,
                                                                free_end=fe, skip_logp=skip)
                    if labels not in best:
                        assert score[0] == -np.inf and (bounds == -1).all() and (ft == -1).all(), (T, labels)
                        continue
                    assert abs(float(score[0]) - best[labels]) <= 1e-5, (T, skip, fs, fe, labels, score[0], best[labels])
                    a, e = bounds[0]
                    assert collapse(ft[0, a:e].tolist()) == list(labels) and (ft[0, :a] == -1).all() and (ft[0, e:] == -1).all()
                    assert (fs or a == 0) and (fe or e == T)


def test_planted_paths_are_recovered_and_a_free_skip_shrinks_the_end_spans():
    rng = np.random.default_rng(2)
    for case in range(100):
        lp, labels, front, tokens = planted_case(rng)
        T = lp.shape[0]
        ft, spans, llp, score, bounds = ref.segment(lp[None], [T], np.array([labels]), [len(labels)], skip_logp=LN_HALF)
        assert bounds[0].tolist() == [front, front + len(tokens)], case
        assert ft[0, front:front + len(tokens)].tolist() == tokens, case
        assert (ft[0, :front] == -1).all() and (ft[0, front + len(tokens):] == -1).all()
    for case in range(20):                                                  # first and last label planted on >= 3 frames each
        lp, labels, front, tokens = planted_case(rng, min_edge_span=3)
        T, L = lp.shape[0], len(labels)
        kept = ref.segment(lp[None], [T], np.array([labels]), [L], skip_logp=LN_HALF)[1][0]
        free = ref.segment(lp[None], [T], np.array([labels]), [L], skip_logp=0.0)[1][0]
        assert kept[0, 1] - kept[0, 0] >= 3 and kept[L - 1, 1] - kept[L - 1, 0] >= 3
        assert free[0, 1] - free[0, 0] == 1 and free[L - 1, 1] - free[L - 1, 0] == 1, case


def test_tie_rules():
    """every log-prob -1 and skip_logp -1 (sums and products exact): every path, start and end scores -T, the tie rules alone decide"""
    T = 7
    lp = np.full((1, T, 3), -1.0, np.float32)
    tg, tl = np.array([UNIFORM_TIE_LABELS]), [3]
    # fixed ends: the smallest step wins among equal predecessors and 2L beats 2L-1 at the end, as in the forced alignment
    ft, spans, _, score, bounds = ref.segment(lp, [T], tg, tl, free_start=False, free_end=False, skip_logp=-1.0)
    assert ft[0].tolist() == UNIFORM_TIE_FRAME_TOKEN and bounds[0].tolist() == [0, T] and score[0] == -T
    # a free start: the virtual start is the last candidate, so staying on the path that began at frame 0 keeps the tie
    ft, _, _, score, bounds = ref.segment(lp, [T], tg, tl, free_start=True, free_end=False, skip_logp=-1.0)
    assert ft[0].tolist() == UNIFORM_TIE_FRAME_TOKEN and bounds[0].tolist() == [0, T] and score[0] == -T
    # a free end: the earliest frame wins, which is frame 3 in state 2L-1 (1, blank, 1, 2 need four frames; 2L is not reached by then)
    for fs in (False, True):
        ft, spans, llp, score, bounds = ref.segment(lp, [T], tg, tl, free_start=fs, free_end=True, skip_logp=-1.0)
        assert ft[0].tolist() == [1, 0, 1, 2, -1, -1, -1] and bounds[0].tolist() == [0, 4] and score[0] == -T
        assert spans[0].tolist() == [[0, 1], [2, 3], [3, 4]] and llp[0].tolist() == [-1.0, -1.0, -1.0]
    # one label on two frames, free end: at frame 0 only 2L-1 is finite; with a fixed end 2L (label, then blank) beats 2L-1 (label twice)
    one = np.array([[1]])
    assert ref.segment(lp, [2], one, [1], free_start=False, free_end=True, skip_logp=-1.0)[0][0, :2].tolist() == [1, -1]
    assert ref.segment(lp, [2], one, [1], free_start=False, free_end=False, skip_logp=-1.0)[0][0, :2].tolist() == [1, 0]
    # infeasible: no labels, no frames, a length beyond max_tgt, too few frames
    for in_len, n in (([T], [0]), ([0], [3]), ([T], [4]), ([3], [3])):
        ft, spans, llp, score, bounds = ref.segment(lp, in_len, tg, n)
        assert score[0] == -np.inf and (ft == -1).all() and (spans == -1).all() and (bounds == -1).all() and (llp == 0).all()


def test_confidence_restatement():
    llp = [-1.0, -4.0, -9.0, -2.0]
    spans = [[0, 1], [1, 3], [3, 6], [6, 7]]
    assert ref.confidence(llp, spans, [4], conf_window=2) == [-2.5]          # m = -1, -2, -3, -2: window means -1.5, -2.5, -2.5
    assert ref.confidence(llp, spans, [1, 3], conf_window=8) == [-1.0, -7.0 / 3.0]


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.otr_ctc_segment_workspace_bytes
    assert ws(1, 1, 1) > 0 and ws(1, 1 << 20, 4095) > 0 and ws(8, 16384, 2048) % 8 == 0
    assert ws(1, 1 << 20, 4095) >= (1 << 20) * 8191 * 2 // 8                 # two bits per frame and state
    assert ws(2, 100, 20) >= 2 * 100 * 41 * 2 // 8
    for bad in ((0, 10, 5), (1, 0, 5), (1, (1 << 20) + 1, 5), (1, 10, 0), (1, 10, 4096), (-1, 10, 5), (1, 10, -1)):
        assert ws(*bad) == -1, bad


def test_entries_refuse_bad_arguments_without_a_gpu_and_leave_the_outputs_alone():
    lib = _lib.load()
    B, T, V, M = 2, 50, 10, 6
    need = lib.otr_ctc_segment_workspace_bytes(B, T, M)
    host = {'lp': np.zeros((B, T, V), np.float32), 'tg': np.ones((B, M), np.int64), 'il': np.full(B, T, np.int32),
            'tl': np.full(B, M, np.int32), 'workspace': np.full(need // 8 + 1, 0x5A5A5A5A, np.int64),
            'ft': np.full((B, T), 77, np.int32), 'sp': np.full((B, M, 2), 78, np.int32), 'll': np.full((B, M), 7.5, np.float32),
            'sc': np.full(B, 8.5, np.float32), 'bd': np.full((B, 2), 79, np.int32)}
    before = {k: v.copy() for k, v in host.items()}
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in host.items()}

    def call(ld=V, ldt=M, B=B, T=T, V=V, max_tgt=M, blank=0, fs=1, fe=1, skip=-0.5, ws_bytes=need, **over):
        a = dict(ptr, **over)
        return lib.otr_ctc_segment(a['lp'], ld, a['tg'], ldt, a['il'], a['tl'], B, T, V, max_tgt, blank, fs, fe, skip, a['workspace'],
                                   ws_bytes, a['ft'], a['sp'], a['ll'], a['sc'], a['bd'], None)

    def refused(why, **kw):
        assert call(**kw) < 0, kw
        msg = lib.otr_last_error_string()
        assert b'ctc_segment' in msg and why in msg, (kw, msg)

    for name in ptr:
        refused(b'null', **{name: None})
    refused(b'shape', B=0)
    refused(b'shape', T=0)
    refused(b'shape', T=(1 << 20) + 1)
    refused(b'shape', V=1, ld=1)
    refused(b'max_tgt', max_tgt=0)
    refused(b'max_tgt', max_tgt=4096, ldt=4096)
    refused(b'ld=', ld=V - 1)
    refused(b'ldt=', ldt=M - 1)
    refused(b'blank', blank=V)
    refused(b'blank', blank=-1)
    refused(b'free_start', fs=2)
    refused(b'free_start', fs=-1)
    refused(b'free_end', fe=2)
    refused(b'skip_logp', skip=0.5)
    refused(b'skip_logp', skip=float('nan'))
    refused(b'skip_logp', skip=float('-inf'))
    refused(b'workspace', ws_bytes=need - 1)
    refused(b'aligned', workspace=C.c_void_p(host['workspace'].ctypes.data + 4))
    for k, v in host.items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)


def test_entries_are_in_the_header_the_binding_and_both_libraries():
    header = open(HEADER).read()
    assert re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1) == '608' and _lib.OTR_ABI_VERSION == 608
    still = header[header.index('still 608'):header.index('#define OTR_ABI_VERSION')]
    for name in ('otr_ctc_segment_workspace_bytes', 'otr_ctc_segment'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SIGNATURES and name in still
        for kind in ('bf16', 'fp16'):
            lib = _lib.load(kind)
            assert lib.otr_version() == 608 and getattr(lib, name) is not None
    assert _lib.load().otr_ctc_segment_workspace_bytes.restype is C.c_int64
    assert len(_lib.SIGNATURES['otr_ctc_segment']) == 22


@pytest.mark.parametrize('window, hop', [(400, 200), (1600, 800), (48, 40), (107, 12)])
def test_window_plan_covers_every_encoder_frame_once(window, hop):
    from opentransformer_amd import ops
    from opentransformer_amd.segment import window_plan
    t2 = lambda n: ops.conv_geometry(n, 80)[2]    # noqa: E731
    for T in (window, window + 1, 5 * hop + 3, hop + 9, window - 1, max(7, window // 3), 7, 3 * window + hop // 2):
        plan = window_plan(T, window, hop)
        seen = np.zeros(t2(T), np.int64)
        for i, (start, length, lo, hi, out) in enumerate(plan):
            assert start == i * hop and 0 < length <= window and start + length <= T
            assert length == window or i == len(plan) - 1                   # only the last window is short
            assert 0 <= lo <= hi <= t2(length), (T, plan)
            assert out == start // 4 + lo                                   # encoder frame k of window i is global frame i*hop/4 + k
            seen[out:out + hi - lo] += 1
            if 0 < i < len(plan) - 1:
                assert hi - lo == hop // 4 and lo == (t2(window) - hop // 4) // 2
        assert (seen == 1).all(), (T, plan)
        assert plan[0][2] == 0 and plan[-1][0] + plan[-1][1] == T and plan[-1][3] == t2(plan[-1][1])
        if T <= window:
            assert len(plan) == 1


def test_window_plan_refuses_bad_windows():
    from opentransformer_amd.segment import CTCSegmenter, window_plan
    for T, window, hop in ((1000, 400, 202), (1000, 400, 0), (1000, 400, -4), (1000, 207, 200), (1000, 200, 200), (6, 400, 200)):
        with pytest.raises(ValueError):
            window_plan(T, window, hop)
    with pytest.raises(ValueError):
        CTCSegmenter(torch.nn.Identity(), window=400, hop=398)


def test_op_refuses_cpu_tensors_and_4096_label_columns():
    from opentransformer_amd import ops
    import opentransformer_amd as ota
    assert ops.CTC_SEGMENT_MAX_TGT == 4095 and ota.CTCSegmenter is not None
    lp, il = torch.zeros(1, 4, 5), torch.tensor([4])
    with pytest.raises(_lib.OtransHipError):
        ops.ctc_segment(lp, il, torch.ones(1, 2, dtype=torch.long), torch.tensor([2]))
    with pytest.raises(ValueError, match='4095'):
        ops.ctc_segment(lp, il, torch.ones(1, 4096, dtype=torch.long), torch.tensor([2]))
    with pytest.raises(ValueError, match='4095'):
        ops.ctc_segment(lp, il, torch.ones(1, 0, dtype=torch.long), torch.tensor([0]))
