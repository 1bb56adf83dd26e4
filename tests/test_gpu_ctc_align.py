"""GPU (-m gpu): CTC forced alignment on the device (otr_ctc_align, ops.ctc_forced_align, the models' and the recognizer's align)
against the numpy restatement tests/ctc_align_ref.py.  Both do one correctly rounded float32 add per frame after an exact max, in the
same order, so frame_token and spans must be identical for every utterance; score and label_logp, for which 1e-6 relative + 1e-6
absolute was the bound to meet, turned out bit-equal in every case and are asserted equal."""
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import ops
from opentransformer_amd import synthetic as syn
from tests import ctc_align_ref as ref
from tests.test_ctc_align import UNIFORM_TIE_FRAME_TOKEN, UNIFORM_TIE_LABELS, collapse

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def device_align(lp, in_len, targets, tgt_len, blank=0):
    out = ops.ctc_forced_align(lp if torch.is_tensor(lp) else torch.from_numpy(lp).to(DEV),
                               torch.tensor(in_len, dtype=torch.int32, device=DEV),
                               torch.as_tensor(np.asarray(targets), dtype=torch.int64).to(DEV),
                               torch.tensor(tgt_len, dtype=torch.int32, device=DEV), blank=blank)
    return [t.cpu().numpy() for t in out]


def check_against_restatement(lp, in_len, targets, tgt_len, blank=0, lp_dev=None):
    """device == restatement for every utterance: frame_token and spans identical, score and label_logp bit-equal; returns the
    device outputs"""
    targets = np.asarray(targets, dtype=np.int64)
    got = device_align(lp if lp_dev is None else lp_dev, in_len, targets, tgt_len, blank)
    want = ref.align(lp, in_len, targets, tgt_len, blank)
    B, T = lp.shape[:2]
    assert got[0].shape == (B, T) and got[1].shape == (B, targets.shape[1], 2) and got[2].shape == (B, targets.shape[1])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and got[3].dtype == np.float32
    for b in range(B):
        np.testing.assert_array_equal(got[0][b], want[0][b], err_msg='frame_token of utterance %d' % b)
        np.testing.assert_array_equal(got[1][b], want[1][b], err_msg='spans of utterance %d' % b)
    fin = np.isfinite(want[3])
    np.testing.assert_array_equal(got[3][~fin], want[3][~fin])
    print('max |score - restatement|', float(np.abs(got[3][fin] - want[3][fin]).max()) if fin.any() else 0.0,
          'max |label_logp - restatement|', float(np.abs(got[2] - want[2]).max()) if got[2].size else 0.0,
          'bit-equal', bool(np.array_equal(got[3], want[3]) and np.array_equal(got[2], want[2])))
    # the bound set for this check is 1e-6 relative + 1e-6 absolute; on the MI355X every case came out bit-equal, so
    # equality is what is asserted
    np.testing.assert_array_equal(got[3], want[3])
    np.testing.assert_array_equal(got[2], want[2])
    return got


def peaky_log_probs(rng, B, T, V, scale=4.0):
    x = torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * scale)
    return torch.log_softmax(x, -1).numpy()


def padded(rows, width=None):
    width = max(1, max(len(r) for r in rows)) if width is None else width
    return np.array([list(r) + [0] * (width - len(r)) for r in rows], dtype=np.int64), [len(r) for r in rows]


@pytest.mark.parametrize('lengths', [[35, 35, 35, 35], [35, 30, 17, 1]])
def test_reference_log_probs(golden, lengths):
    """the CTC head's log-probs the real reference produced (tests/golden/c1_decode.npz): the greedy collapse of each row, a
    sequence that is not the greedy one, and no labels at all"""
    lp = golden('c1_decode.npz')['ctc_head_logp'].astype(np.float32)        # [4, 35, 100]
    greedy = [collapse(lp[b, :n].argmax(-1).tolist()) for b, n in enumerate(lengths)]
    tg, tl = padded(greedy)
    got = check_against_restatement(lp, lengths, tg, tl)
    for b, n in enumerate(lengths):                                         # the greedy path is the best path of its own collapse
        assert got[0][b, :n].tolist() == lp[b, :n].argmax(-1).tolist()
    other = [[5, 7, 7, 9], [2, 2, 2], [98, 3, 99, 3, 3, 4, 50], [6]]
    assert all(o != g for o, g in zip(other, greedy))
    tg, tl = padded(other)
    check_against_restatement(lp, lengths, tg, tl)
    got = check_against_restatement(lp, lengths, np.zeros((4, 3), np.int64), [0, 0, 0, 0])
    for b, n in enumerate(lengths):
        assert (got[0][b, :n] == 0).all() and (got[1][b] == -1).all()


def test_wave_boundaries_of_the_state_axis():
    """S = 2L+1 states on up to 256 threads: L around every wave edge, all four waves at L = 127"""
    rng = np.random.default_rng(1)
    V, T = 50, 300
    Ls = [0, 1, 31, 32, 33, 63, 64, 95, 96, 127]
    lp = peaky_log_probs(rng, len(Ls), T, V, scale=2.0)
    rows = []
    for L in Ls:
        r = rng.integers(1, V, size=L)
        r[rng.random(L) < 0.2] = 7                                           # adjacent repeats here and there
        rows.append(r.tolist())
    tg, tl = padded(rows, 127)
    got = check_against_restatement(lp, [T] * len(Ls), tg, tl)
    assert np.isfinite(got[3]).all()
    tg2, tl2 = padded(rows[:4], 33)                                          # a narrower workgroup (two waves) for the same rows
    got2 = check_against_restatement(lp[:4], [T, 250, T, 299], tg2, tl2)
    np.testing.assert_array_equal(got2[0][2], got[0][2])


def test_feasibility_edges():
    rng = np.random.default_rng(2)
    V, T = 20, 24
    plain = list(range(1, 13))                                               # 12 labels, no repeats
    rep = [3, 3, 4, 5, 5, 5, 6, 7, 8, 9]                                     # 10 labels, r = 3 adjacent repeats
    rows = [plain, rep, rep, [1, 2, 3], [], [4], [], [1, 2, 3, 4, 5], [1, 2], [1, 2], plain]
    in_len = [12, 13, 12, 0, 0, 1, 1, T, T, 1, T]
    tg, tl = padded(rows, 12)
    tl[8] = 13                                                               # a target length beyond max_tgt
    lp = peaky_log_probs(rng, len(rows), T, V, scale=2.0)
    got = check_against_restatement(lp, in_len, tg, tl)
    ft, spans, llp, score = got
    assert ft[0, :12].tolist() == plain and (ft[0, 12:] == -1).all()         # T = L: no blank on the path
    assert ft[1, :13].tolist() == [3, 0, 3, 4, 5, 0, 5, 0, 5, 6, 7, 8, 9]    # T = L + r: blanks between the repeats only
    for b in (2, 3, 8, 9):                                                   # T = L + r - 1, no frames, bad length, 1 frame for 2 labels
        assert score[b] == -math.inf and (ft[b] == -1).all() and (spans[b] == -1).all() and (llp[b] == 0).all(), b
    assert score[4] == 0.0 and (ft[4] == -1).all() and (spans[4] == -1).all()           # no frames, no labels: the empty path
    assert ft[5, 0] == 4 and spans[5, 0].tolist() == [0, 1] and score[5] == lp[5, 0, 4] and llp[5, 0] == lp[5, 0, 4]
    assert ft[6, 0] == 0 and score[6] == lp[6, 0, 0]
    assert np.isfinite(score[[7, 10]]).all()


@pytest.mark.parametrize('T', [960, 961, 2048])
def test_both_back_pointer_routes(T):
    """back-pointers in LDS up to T = 960, in the workspace above"""
    from opentransformer_amd import _lib
    lib = _lib.load()
    assert lib.otr_ctc_align_workspace_bytes(2, 960, 10) == 8 and lib.otr_ctc_align_workspace_bytes(2, 961, 10) == 2 * 961 * 64
    rng = np.random.default_rng(T)
    B, V, L = 2, 20, 10
    lp = peaky_log_probs(rng, B, T, V, scale=1.0)
    tg = rng.integers(1, V, size=(B, L))
    tg[1, 4] = tg[1, 3]
    got = check_against_restatement(lp, [T, T - 37], tg, [L, L - 1])
    assert np.isfinite(got[3]).all() and (got[0][1, T - 37:] == -1).all()


def test_large_vocabulary_in_a_row_padded_view():
    rng = np.random.default_rng(4)
    B, T, V, L = 3, 64, 4233, 20
    lp = peaky_log_probs(rng, B, T, V)
    buf = torch.full((B, T, V + 7), float('nan'), device=DEV)
    buf[:, :, :V] = torch.from_numpy(lp).to(DEV)
    view = buf[:, :, :V]
    assert view.stride(1) == V + 7 and not view.is_contiguous()
    tg = rng.integers(1, V, size=(B, L))
    tg[0, 0], tg[0, 1] = V - 1, V - 1
    got = check_against_restatement(lp, [T, 50, 41], tg, [L, L, L - 3], lp_dev=view)
    assert np.isfinite(got[3]).all()


def test_tie_rule_on_the_device():
    lp = np.full((1, 7, 3), np.log(1.0 / 3.0), np.float32)
    got = check_against_restatement(lp, [7], np.array([UNIFORM_TIE_LABELS]), [3])
    assert got[0][0].tolist() == UNIFORM_TIE_FRAME_TOKEN
    assert got[1][0].tolist() == [[0, 1], [2, 3], [3, 4]]


def test_cross_checks_without_the_restatement():
    rng = np.random.default_rng(6)
    B, T, V = 6, 80, 30
    lp = peaky_log_probs(rng, B, T, V, scale=3.0)
    in_len = [80, 71, 64, 33, 80, 50]
    rows = [rng.integers(1, V, size=n).tolist() for n in (12, 9, 20, 5, 1, 14)]
    rows[2][5] = rows[2][4]
    tg, tl = padded(rows)
    x = torch.from_numpy(lp).to(DEV)
    ft, spans, llp, score = device_align(x, in_len, tg, tl)
    for b in range(B):
        n, labels = in_len[b], rows[b]
        path = ft[b, :n].tolist()
        assert collapse(path) == labels and (ft[b, n:] == -1).all()
        along = float(sum(np.float64(lp[b, t, c]) for t, c in enumerate(path)))
        assert abs(along - float(score[b])) <= 1e-5 * abs(along), (b, along, score[b])
        with torch.no_grad():                                                # the loss sums every path: never below the best one
            loss = ops.CTCLossFn.apply(x[b:b + 1, :n].contiguous(), torch.tensor([labels], device=DEV),
                                       torch.tensor([n], device=DEV), torch.tensor([len(labels)], device=DEV), 0)
        nll = float(loss) * max(len(labels), 1)
        assert float(score[b]) <= -nll + 1e-4, (b, score[b], nll)
        end = 0
        for j, c in enumerate(labels):
            a, e = spans[b, j]
            assert end <= a < e <= n, (b, j, spans[b])                       # non-empty, ordered, no overlap
            assert all(path[t] == c for t in range(a, e))
            assert (a == 0 or path[a - 1] != c) and (e == n or path[e] != c)     # the whole run of the label's state
            want = float(sum(np.float64(lp[b, t, c]) for t in range(a, e)))
            assert abs(float(llp[b, j]) - want) <= 1e-5 * abs(want) + 1e-6
            end = e
        assert (spans[b, len(labels):] == -1).all() and (llp[b, len(labels):] == 0).all()


def test_models_align_what_their_ctc_term_is_trained_on(golden):
    """SpeechToText aligns labels + [EOS] and drops the EOS column; CTCModel aligns the labels as they are"""
    import opentransformer_amd as ota
    from opentransformer_amd.nn import EOS
    from tests.test_gpu_ctc_beam import load_c1
    g = golden('c1_decode.npz')
    try:
        model = load_c1(g, 'fp32')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        labels = torch.tensor([[5, 6, 7, 8, 9], [12, 12, 30, 0, 0], [40, 41, 42, 43, 0], [0, 0, 0, 0, 0]], device=DEV)
        n = torch.tensor([5, 3, 4, 0], device=DEV)
        ft, spans, llp, score = model.align(x, m, labels, n)
        with torch.no_grad():
            fx, fm = model.frontend(x, m)
            memory, memory_mask, _ = model.encoder(fx, fm)
            log_probs, length = model.assistor.inference(memory, memory_mask)
        ext = torch.tensor([[5, 6, 7, 8, 9, EOS], [12, 12, 30, EOS, 0, 0], [40, 41, 42, 43, EOS, 0], [EOS, 0, 0, 0, 0, 0]], device=DEV)
        ft2, spans2, llp2, score2 = ops.ctc_forced_align(log_probs, length, ext, n + 1)
        assert torch.isfinite(score).all() and spans.shape == (4, 5, 2) and llp.shape == (4, 5)
        assert torch.equal(ft, ft2) and torch.equal(score, score2)
        for b in range(4):
            k = int(n[b])
            assert torch.equal(spans[b, :k], spans2[b, :k]) and torch.equal(llp[b, :k], llp2[b, :k])
            assert (spans[b, k:] == -1).all() and (llp[b, k:] == 0).all()
            assert int(spans2[b, k, 1]) > int(spans2[b, k, 0]) >= 0                     # the EOS was on the path
        cfg = syn.c1_model(0.0, ctc_weight=0.3)
        cm = ota.CTCModel(dict(cfg, vocab_size=cfg['decoder']['vocab_size'], lookahead_steps=2))
        syn.fill_state_dict_(cm.state_dict(), 21)
        cm = cm.to(DEV).eval()
        got = cm.align(x, m, labels, n)
        log_probs, length = cm.inference(x, m)
        want = ops.ctc_forced_align(log_probs, length, labels, n)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.isfinite(got[3]).all()
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['greedy', 'beam'])
def test_recognizer_time_stamps(golden, mode):
    from opentransformer_amd.recognize import CTCRecognizer
    from tests.test_gpu_ctc_beam import load_c1
    g = golden('c1_decode.npz')
    try:
        model = load_c1(g, 'fp32')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        idx2unit = {i: 'u%d' % i for i in range(100)}
        rec = CTCRecognizer(model, idx2unit=idx2unit, mode=mode, beam_width=5)
        texts, times = rec.recognize_with_times(x, m)
        assert texts == rec.recognize(x, m) and len(times) == 4 and any(texts)
        frames = g['mask'].shape[1]
        for text, items in zip(texts, times):
            assert ' '.join(u for u, _, _, _ in items) == text
            end = 0
            for _, a, e, logp in items:
                assert end <= a < e <= frames and logp <= 0.0
                end = e
        # a known transcript through the recognizer: the same spans as the model's own alignment
        labels = torch.tensor([[5, 6, 7], [12, 12, 0]], device=DEV)
        n = torch.tensor([3, 2], device=DEV)
        items = rec.align(x[:2], m[:2], labels, n)
        with torch.no_grad():
            fx, fm = model.frontend(x[:2], m[:2])
            memory, memory_mask, _ = model.encoder(fx, fm)
            _, spans, llp, _ = model.assistor.align(memory, memory_mask, labels, n)
        assert [[u for u, _, _, _ in it] for it in items] == [['u5', 'u6', 'u7'], ['u12', 'u12']]
        assert [[[a, e] for _, a, e, _ in it] for it in items] == [spans[b, :int(n[b])].tolist() for b in range(2)]
        assert items[1][1][3] == float(llp[1, 1])
    finally:
        ops.set_compute_dtype('bf16')
