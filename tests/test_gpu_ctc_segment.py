"""GPU (-m gpu): CTC segmentation on the device (otr_ctc_segment, ops.ctc_segment, segment.CTCSegmenter) against the numpy restatement
tests/ctc_segment_ref.py.  Both sides do the same single float32 operations in the same order (one multiply for a skipped stretch, an
exact max, one add per frame), so frame_token, spans and bounds must be identical and score and label_logp bit-equal."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, ops
from opentransformer_amd import synthetic as syn
from tests import ctc_segment_ref as ref
from tests.test_ctc_segment import LN_HALF, planted_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('frame_token', 'spans', 'label_logp', 'score', 'bounds')


def device_segment(lp, in_len, targets, tgt_len, **kw):
    out = ops.ctc_segment(lp if torch.is_tensor(lp) else torch.from_numpy(lp).to(DEV),
                          torch.tensor(in_len, dtype=torch.int32, device=DEV),
                          torch.as_tensor(np.asarray(targets), dtype=torch.int64).to(DEV),
                          torch.tensor(tgt_len, dtype=torch.int32, device=DEV), **kw)
    return [t.cpu().numpy() for t in out]


def check_against_restatement(lp, in_len, targets, tgt_len, lp_dev=None, **kw):
    """device == restatement for every recording and every output, bit for bit; returns the device outputs"""
    targets = np.asarray(targets, dtype=np.int64)
    got = device_segment(lp if lp_dev is None else lp_dev, in_len, targets, tgt_len, **kw)
    want = ref.segment(lp, in_len, targets, tgt_len, **kw)
    B, T = lp.shape[:2]
    M = targets.shape[1]
    assert [g.shape for g in got] == [(B, T), (B, M, 2), (B, M), (B,), (B, 2)]
    assert [g.dtype for g in got] == [np.int32, np.int32, np.float32, np.float32, np.int32]
    fin = np.isfinite(want[3])
    print('max |score - restatement|', float(np.abs(got[3][fin] - want[3][fin]).max()) if fin.any() else 0.0,
          'max |label_logp - restatement|', float(np.abs(got[2] - want[2]).max()))
    for b in range(B):
        for name, g, w in zip(NAMES, got, want):
            np.testing.assert_array_equal(g[b], w[b], err_msg='%s of recording %d' % (name, b))
    return got


def peaky_log_probs(rng, B, T, V, scale=4.0):
    x = torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * scale)
    return torch.log_softmax(x, -1).numpy()


def padded(rows, width=None):
    width = max(1, max(len(r) for r in rows)) if width is None else width
    return np.array([list(r) + [0] * (width - len(r)) for r in rows], dtype=np.int64), [len(r) for r in rows]


def random_labels(rng, L, V, repeat=0.2):
    r = rng.integers(1, V, size=L)
    r[rng.random(L) < repeat] = 1
    return r.tolist()


def repeats(row):
    return sum(a == b for a, b in zip(row[1:], row[:-1]))


def test_fixed_ends_equal_forced_alignment():
    rng = np.random.default_rng(0)
    B, T, V = 4, 96, 12
    lp = peaky_log_probs(rng, B, T, V, scale=2.0)
    rows = [random_labels(rng, L, V) for L in (40, 17, 1, 5)]
    in_len = [96, 80, 96, 33]
    tg, tl = padded(rows, 127)
    got = check_against_restatement(lp, in_len, tg, tl, free_start=False, free_end=False, skip_logp=LN_HALF)
    x = torch.from_numpy(lp).to(DEV)
    want = ops.ctc_forced_align(x, torch.tensor(in_len, dtype=torch.int32, device=DEV), torch.from_numpy(tg).to(DEV),
                                torch.tensor(tl, dtype=torch.int32, device=DEV))
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w.cpu().numpy(), err_msg=name)
    assert np.isfinite(got[3]).all() and got[4].tolist() == [[0, n] for n in in_len]


@pytest.mark.parametrize('free_start, free_end, skip_logp', [(True, True, 0.0), (True, True, LN_HALF), (True, False, LN_HALF),
                                                            (False, True, LN_HALF), (True, False, 0.0), (False, True, 0.0)])
def test_free_ends_on_a_ragged_batch(free_start, free_end, skip_logp):
    rng = np.random.default_rng(1)
    B, T, V = 3, 300, 9
    lp = peaky_log_probs(rng, B, T, V, scale=1.5)
    rows = [random_labels(rng, L, V, repeat=0.1) for L in (130, 40, 1)]
    in_len = [300, 257, 131]
    tg, tl = padded(rows)
    got = check_against_restatement(lp, in_len, tg, tl, free_start=free_start, free_end=free_end, skip_logp=skip_logp)
    assert np.isfinite(got[3]).all()
    for b, n in enumerate(in_len):
        a, e = got[4][b]
        assert 0 <= a < e <= n and (free_start or a == 0) and (free_end or e == n)
        assert (got[0][b, :a] == -1).all() and (got[0][b, e:] == -1).all() and (got[0][b, a:e] >= 0).all()


@pytest.mark.parametrize('L', [127, 128, 511, 512, 1023, 1024, 2047, 2048, 4095])
def test_strip_and_wave_edges(L):
    """one recording each, max_tgt = L: S = 2L+1 straddles a wave (255 / 257 states on strips of 4), the 256-thread variant's last
    size and the next one's first (1023 / 1025), 2048, the step from strips of 4 to strips of 8 (4095 / 4097) and ends at 8191.  V = 6:
    adjacent repeats are frequent, so the s-2 rule matters at strip borders"""
    rng = np.random.default_rng(L)
    V = 6
    row = rng.integers(1, V, size=L).tolist()
    T = L + repeats(row) + 64
    assert repeats(row) > L // 10
    lp = peaky_log_probs(rng, 1, T, V, scale=1.0)
    tg, tl = padded([row])
    got = check_against_restatement(lp, [T], tg, tl, skip_logp=LN_HALF)
    assert np.isfinite(got[3]).all()
    got = check_against_restatement(lp, [T - 3], tg, tl, free_start=False, free_end=False)
    assert got[4].tolist() == [[0, T - 3]]


def test_end_state_at_every_place_of_a_strip():
    """L < max_tgt: the owner of state 2L holds it at place 2L mod R of its strip, R = 4 (max_tgt 1030) and R = 8 (max_tgt 2100)"""
    rng = np.random.default_rng(5)
    V = 6
    for max_tgt, Ls in ((1030, (600, 601)), (2100, (1200, 1201, 1202, 1203))):
        rows = [rng.integers(1, V, size=L).tolist() for L in Ls]
        T = max(L + repeats(r) for L, r in zip(Ls, rows)) + 40
        lp = peaky_log_probs(rng, len(Ls), T, V, scale=1.0)
        tg, tl = padded(rows, max_tgt)
        got = check_against_restatement(lp, [T] * len(Ls), tg, tl, skip_logp=LN_HALF)
        assert np.isfinite(got[3]).all()


@pytest.mark.parametrize('T', [5000, 4096, 4097])
def test_long_stays(T):
    """30 labels over thousands of frames: the back-trace crosses many of its 64-frame blocks with the state standing still; T a
    multiple of the block and of every prefetch depth (4096), one more, and neither (5000)"""
    rng = np.random.default_rng(T)
    B, V, L = 2, 12, 30
    lp = peaky_log_probs(rng, B, T, V, scale=1.0)
    rows = [random_labels(rng, L, V), random_labels(rng, L - 1, V)]
    tg, tl = padded(rows)
    got = check_against_restatement(lp, [T, T - 37], tg, tl, skip_logp=LN_HALF)
    assert np.isfinite(got[3]).all() and (got[0][1, T - 37:] == -1).all()
    check_against_restatement(lp, [T, T - 37], tg, tl, free_start=False, free_end=False)


def test_planted_paths_are_recovered():
    rng = np.random.default_rng(2)
    cases = [planted_case(rng) for _ in range(16)]
    T = max(c[0].shape[0] for c in cases)
    lp = np.full((len(cases), T, 8), np.float32(math.log(1.0 / 8)), np.float32)
    for b, c in enumerate(cases):
        lp[b, :c[0].shape[0]] = c[0]
    tg, tl = padded([c[1] for c in cases])
    got = check_against_restatement(lp, [c[0].shape[0] for c in cases], tg, tl, skip_logp=LN_HALF)
    for b, (_, labels, front, tokens) in enumerate(cases):
        assert got[4][b].tolist() == [front, front + len(tokens)]
        assert got[0][b, front:front + len(tokens)].tolist() == tokens


def test_infeasible_rows_inside_a_batch():
    rng = np.random.default_rng(3)
    T, V, M = 40, 7, 12
    rep = [3, 3, 4, 5, 5, 5, 6, 2, 1, 2]                                     # 10 labels, 3 adjacent repeats: 13 frames at least
    rows = [[1, 2, 3, 4], rep, [1, 2, 3], [], [1, 2], [1, 2, V], [1, -1, 2], [1, 2, 3], rep, [4, 5, 6]]
    in_len = [T, 12, 0, T, T, T, T, T, 13, 33]
    tg, tl = padded(rows, M)
    tl[4] = M + 1                                                            # a target length beyond max_tgt
    lp = peaky_log_probs(rng, len(rows), T, V, scale=2.0)
    lp[7, :, 2] = -np.inf                                                    # label 2 is on every path of recording 7
    lp[9, 5:20, 0] = -np.inf                                                 # feasible all the same: the path need not pass there as blank
    got = check_against_restatement(lp, in_len, tg, tl, skip_logp=LN_HALF)
    ft, spans, llp, score, bounds = got
    for b in (1, 2, 3, 4, 5, 6, 7):
        assert score[b] == -math.inf and (ft[b] == -1).all() and (spans[b] == -1).all() and (llp[b] == 0).all() and (bounds[b] == -1).all(), b
    assert np.isfinite(score[[0, 8, 9]]).all() and bounds[8].tolist() == [0, 13]
    keep = [0, 8, 9]                                                         # the neighbours, alone in a batch: unchanged
    alone = device_segment(lp[keep], [in_len[b] for b in keep], tg[keep], [tl[b] for b in keep], skip_logp=LN_HALF)
    for name, g, a in zip(NAMES, got, alone):
        np.testing.assert_array_equal(g[keep], a, err_msg=name)


def raw_call(lp, in_len, tg, tl, ws, outs, V=None, max_tgt=None, blank=0, skip=LN_HALF, ws_bytes=None):
    B, T = lp.shape[:2]
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    ret = _lib.load().otr_ctc_segment(p(lp), lp.stride(1), p(tg), tg.stride(0), p(in_len), p(tl), B, T, lp.shape[2] if V is None else V,
                                      tg.shape[1] if max_tgt is None else max_tgt, blank, 1, 1, skip, p(ws),
                                      ws.numel() * ws.element_size() if ws_bytes is None else ws_bytes, *[p(o) for o in outs],
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ret


def test_hygiene():
    """frames past the length are not read, the workspace need not be zeroed and can be used again, a row-padded view is read in
    place, a refused call leaves the outputs alone"""
    rng = np.random.default_rng(4)
    B, T, V, M = 3, 200, 11, 70
    in_len = [200, 150, 77]
    lp = peaky_log_probs(rng, B, T, V, scale=1.5)
    rows = [random_labels(rng, L, V) for L in (70, 33, 8)]
    tg, tl = padded(rows, M)
    buf = torch.full((B, T, V + 5), float('nan'), device=DEV)
    buf[:, :, :V] = torch.from_numpy(lp).to(DEV)
    for b, n in enumerate(in_len):
        buf[b, n:] = float('nan')
    view = buf[:, :, :V]
    assert view.stride(1) == V + 5 and not view.is_contiguous()
    want = check_against_restatement(lp, in_len, tg, tl, lp_dev=view, skip_logp=LN_HALF)

    need = _lib.load().otr_ctc_segment_workspace_bytes(B, T, M)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    il, tgd, tld = (torch.tensor(in_len, dtype=torch.int32, device=DEV), torch.from_numpy(tg).to(DEV),
                    torch.tensor(tl, dtype=torch.int32, device=DEV))

    def fresh():
        return [torch.full((B, T), 77, dtype=torch.int32, device=DEV), torch.full((B, M, 2), 78, dtype=torch.int32, device=DEV),
                torch.full((B, M), 7.5, device=DEV), torch.full((B,), 8.5, device=DEV), torch.full((B, 2), 79, dtype=torch.int32, device=DEV)]
    for _ in range(2):                                                       # a workspace of 0xFF bytes, then the one the first call left
        outs = fresh()
        assert raw_call(view, il, tgd, tld, ws, outs) == 0
        for name, o, w in zip(NAMES, outs, want):
            np.testing.assert_array_equal(o.cpu().numpy(), w, err_msg=name)
    outs = fresh()
    filled = [o.clone() for o in outs]
    assert raw_call(view, il, tgd, tld, ws, outs, skip=0.5) < 0
    assert raw_call(view, il, tgd, tld, ws, outs, blank=V) < 0
    assert raw_call(view, il, tgd, tld, ws, outs, ws_bytes=need - 1) < 0 and b'workspace' in _lib.load().otr_last_error_string()
    assert all(torch.equal(o, f) for o, f in zip(outs, filled))


def test_segmenter():
    import opentransformer_amd as ota
    from opentransformer_amd.segment import window_plan
    try:
        ops.set_compute_dtype('fp32')
        model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
        syn.fill_state_dict_(model.state_dict(), 31)
        model = model.to(DEV).eval()
        rng = np.random.default_rng(7)
        T, F, window, hop = 1300, 80, 400, 200
        feats = torch.from_numpy(rng.normal(size=(T, F)).astype(np.float32)).to(DEV)
        seg = ota.CTCSegmenter(model, window=window, hop=hop, skip_logp=LN_HALF, conf_window=8)
        plan = window_plan(T, window, hop)
        assert len(plan) == 6
        x = torch.zeros((len(plan), window, F), device=DEV)
        mask = torch.zeros((len(plan), window), dtype=torch.bool, device=DEV)
        for i, (start, length, _, _, _) in enumerate(plan):
            x[i, :length], mask[i, :length] = feats[start:start + length], True
        with torch.no_grad():
            fx, fm, _ = model.frontend.inference(x, mask, None)
            memory, memory_mask, _ = model.encoder(fx, fm)
            lp_win, length = model.assistor.inference(memory, memory_mask)
        # the kept frames are live frames of their window (the mask of a padded window also counts the frame that straddles its end)
        assert all(int(n) >= hi for n, (_, _, _, hi, _) in zip(length.tolist(), plan))
        lp = seg.log_probs(feats)
        T2 = ops.conv_geometry(T, F)[2]
        assert lp.shape == (T2, 100) and lp.dtype == torch.float32
        for i, (_, _, lo, hi, out) in enumerate(plan):
            assert torch.equal(lp[out:out + hi - lo], lp_win[i, lo:hi].float()), i

        utts = [rng.integers(4, 100, size=n).tolist() for n in (5, 12, 3)]
        res = seg.segment(feats, utts)
        flat = [c for u in utts for c in u]
        ft, spans, llp, score, bounds = [t.cpu().numpy() for t in ops.ctc_segment(
            lp.unsqueeze(0), torch.tensor([T2], dtype=torch.int32, device=DEV), torch.tensor([flat], device=DEV),
            torch.tensor([len(flat)], dtype=torch.int32, device=DEV), blank=model.assistor.blank, skip_logp=LN_HALF)]
        assert np.isfinite(score[0]) and len(res) == 3
        conf = ref.confidence(llp[0], spans[0], [len(u) for u in utts], conf_window=8)
        at = 0
        for u, (start, end, c, items) in zip(utts, res):
            assert [i[0] for i in items] == u
            assert [[i[1], i[2]] for i in items] == spans[0, at:at + len(u)].tolist()
            assert [i[3] for i in items] == llp[0, at:at + len(u)].tolist()
            assert (start, end) == (items[0][1], items[-1][2]) and bounds[0, 0] <= start < end <= bounds[0, 1]
            at += len(u)
        np.testing.assert_allclose([r[2] for r in res], conf, rtol=1e-5, atol=1e-6)
        with pytest.raises(ValueError, match='4095'):
            seg.segment(feats, [[5] * 4000, [6] * 96])
        short = seg.segment(feats[:30], utts)                                # 6 encoder frames for 20 labels: infeasible
        assert short == [None, None, None]
    finally:
        ops.set_compute_dtype('bf16')
