"""GPU (-m gpu): otr_edit_distance / ops.edit_distance / evaluate.ErrorRateMeter against the restatement tests/edit_distance_ref.py.
Everything is integer: dist, counts and totals must be array-equal, for every pair."""
import numpy as np
import pytest
import torch

from opentransformer_amd import evaluate, ops
from tests import edit_distance_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRID = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)          # lengths around the 64-column chunk of a wave and its multiples


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def run(r, rl, h, hl=None, eos=-1, totals=None):
    """the op on numpy inputs -> numpy (dist, counts, totals)"""
    out = ops.edit_distance(dev(r), dev(rl, torch.int32), dev(h), None if hl is None else dev(hl, torch.int32), eos=eos, totals=totals)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int32 and out[2].dtype == torch.int64
    return [t.cpu().numpy() for t in out]


def check(r, rl, h, hl=None, eos=-1, fn=ref.pair):
    got, want = run(r, rl, h, hl, eos), ref.batch(r, rl, h, hl, eos, fn=fn)
    for g, w, name in zip(got, want, ('dist', 'counts', 'totals')):
        np.testing.assert_array_equal(g, w, err_msg=name)
    ok = want[0] >= 0
    assert (got[1].sum(-1)[ok] == got[0][ok]).all()         # S + D + I == dist
    return got


def length_grid(alphabet, seed):
    """all 100 (reference, hypothesis) length pairs of GRID as one B = 100, N = 1 batch"""
    rng = np.random.default_rng(seed)
    rl = np.repeat(GRID, len(GRID))
    hl = np.tile(GRID, len(GRID))
    r = rng.integers(0, alphabet, size=(100, max(GRID)))
    h = rng.integers(0, alphabet, size=(100, 1, max(GRID)))
    return r, rl, h, hl.reshape(100, 1)


@pytest.fixture(scope='module')
def grids():
    """per alphabet: the inputs and the restatement's results, computed once"""
    out = {}
    for alphabet in (2, 50):
        g = length_grid(alphabet, alphabet)
        out[alphabet] = (g, ref.batch(*g))
    return out


@pytest.mark.parametrize('alphabet', [2, 50])
def test_length_grid(grids, alphabet):
    """alphabet 2: many alignments of equal cost, so the tie rule and the carry between chunks decide the counts"""
    (r, rl, h, hl), want = grids[alphabet]
    got = run(r, rl, h, hl)
    for g, w, name in zip(got, want, ('dist', 'counts', 'totals')):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert (got[1].sum(-1) == got[0]).all() and want[2][0] == 100 and want[2][7] == 0


@pytest.mark.parametrize('alphabet', [2, 50])
def test_padding_is_never_read(grids, alphabet):
    (r, rl, h, hl), want = grids[alphabet]
    cols = np.arange(max(GRID))
    # every position at or past a length holds the token that would match there (the other sequence's), then -1
    r_match, h_match = np.where(cols[None] >= rl[:, None], h[:, 0], r), np.where(cols[None] >= hl, r, h[:, 0])[:, None]
    r_neg, h_neg = np.where(cols[None] >= rl[:, None], -1, r), np.where(cols[None] >= hl, -1, h[:, 0])[:, None]
    for rr, hh in ((r_match, h_match), (r_neg, h_neg)):
        got = run(rr, rl, hh, hl)
        for g, w, name in zip(got, want, ('dist', 'counts', 'totals')):
            np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize('N', [1, 3, 10, 32])
def test_nbest_layout_and_strided_views(N):
    rng = np.random.default_rng(N)
    B, Lr, Lh = 5, 40, 45
    wide_h = torch.from_numpy(rng.integers(0, 6, size=(B, 32, Lh + 7))).to(DEV)
    wide_r = torch.from_numpy(rng.integers(0, 6, size=(2 * B, Lr + 3))).to(DEV)
    h, r = wide_h[:, :N, 3:3 + Lh], wide_r[::2, 1:1 + Lr]                     # non-contiguous views, last dimension contiguous
    assert not h.is_contiguous() and not r.is_contiguous()
    rl = rng.integers(0, Lr + 1, size=B)
    hl = rng.integers(0, Lh + 1, size=(B, N))
    hl[0, 0] = rl[0] + 3                                                     # the 1-best is not the oracle where another is nearer
    out = ops.edit_distance(r, dev(rl, torch.int32), h, dev(hl, torch.int32))
    got = [t.cpu().numpy() for t in out]
    assert got[0].shape == (B, N) and got[1].shape == (B, N, 3) and got[2].shape == (8,)
    want = ref.batch(r.cpu().numpy(), rl, h.cpu().numpy(), hl)
    for g, w, name in zip(got, want, ('dist', 'counts', 'totals')):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert got[2][6] == got[0].min(1).sum()                                  # the oracle column
    assert got[2][2] == got[0][:, 0].sum() and (got[2][3:6] == got[1][:, 0].sum(0)).all()    # hypothesis 0 alone feeds the 1-best
    if N > 1:
        assert got[2][6] < got[2][2]


def test_eos_cut():
    E = 7
    rng = np.random.default_rng(3)
    B, L = 6, 70
    r = rng.integers(0, 5, size=(B, L))
    rl = np.full(B, L)
    h = r.copy()[:, None, :]
    hl = np.array([[L], [L], [40], [L], [40], [66]])
    h[0, 0, 0] = E                      # at position 0: the empty hypothesis
    h[1, 0, 33] = E                     # in the middle
    h[2, 0, 39] = E                     # exactly at hyp_len - 1
    #                                     utterance 3: absent
    h[4, 0, 50] = E                     # beyond hyp_len: must be ignored
    h[5, 0, 64] = E                     # in the second chunk of 64 columns
    h[5, 0, 65] = E
    got = check(r, rl, h, hl, eos=E)
    assert got[0][:, 0].tolist() == [L, L - 33, L - 39, 0, L - 40, L - 64]
    check(r, rl, h, hl, eos=-1)         # without eos the token is an ordinary one
    check(r, rl, h, None, eos=E)        # hyp_len=None: the full width, the eos alone ends a hypothesis
    for rt, ht in ((torch.int32, torch.int32), (torch.int32, torch.int64), (torch.int64, torch.int32)):
        out = ops.edit_distance(dev(r, rt), dev(rl, torch.int32), dev(h[:, 0], ht), None, eos=E)     # [B, Lh]: N = 1
        assert out[0].shape == (B, 1) and out[1].shape == (B, 1, 3)
        want = ref.batch(r, rl, h, None, E)
        for g, w in zip(out, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w)


def test_invalid_lengths():
    rng = np.random.default_rng(4)
    B, N, Lr, Lh = 6, 3, 20, 24
    r = rng.integers(0, 4, size=(B, Lr))
    h = rng.integers(0, 4, size=(B, N, Lh))
    rl = np.array([20, -1, Lr + 1, 12, 7, 20])
    hl = rng.integers(0, Lh + 1, size=(B, N))
    hl[3, 0] = Lh + 1                   # hypothesis 0 invalid: the utterance is bad, its other pairs are still scored
    hl[4, 2] = -3                       # hypothesis 2 only: left out of the oracle
    got = check(r, rl, h, hl)
    assert (got[0][1:3] == -1).all() and (got[1][1:3] == -1).all() and got[0][3, 0] == -1 and got[0][4, 2] == -1
    assert (got[0][3, 1:] >= 0).all() and (got[0][4, :2] >= 0).all() and got[2][7] == 3 and got[2][0] == 3
    good = [0, 4, 5]                    # the other utterances' totals are what they are alone
    alone = ref.batch(r[good], rl[good], h[good], hl[good])[2]
    np.testing.assert_array_equal(got[2][:7], alone[:7])


def test_meter_accumulates_and_resets():
    rng = np.random.default_rng(5)
    calls = []
    for B, N in ((4, 2), (3, 5)):
        r, h = rng.integers(0, 3, size=(B, 30)), rng.integers(0, 3, size=(B, N, 33))
        calls.append((r, rng.integers(0, 31, size=B), h, rng.integers(0, 34, size=(B, N))))
    meter = evaluate.ErrorRateMeter(DEV)
    want = np.zeros(8, np.int64)
    for c in calls:
        dist, counts = meter.update(dev(c[0]), dev(c[1], torch.int32), dev(c[2]), dev(c[3], torch.int32))
        fresh = evaluate.ErrorRateMeter(DEV)
        fresh.update(dev(c[0]), dev(c[1], torch.int32), dev(c[2]), dev(c[3], torch.int32))
        w = ref.batch(*c)
        np.testing.assert_array_equal(fresh.totals.cpu().numpy(), w[2])
        np.testing.assert_array_equal(dist.cpu().numpy(), w[0])
        np.testing.assert_array_equal(counts.cpu().numpy(), w[1])
        want += w[2]
    np.testing.assert_array_equal(meter.totals.cpu().numpy(), want)
    res = meter.result()
    assert res['utterances'] == 7 and res['errors'] == want[2] and res['wer'] == want[2] / want[1] * 100
    assert res['topn_wer'] == want[6] / want[1] * 100 and res['substitutions'] + res['deletions'] + res['insertions'] == res['errors']
    meter.reset()
    assert meter.totals.tolist() == [0] * 8


def test_graph_capture_replays_add_to_totals():
    rng = np.random.default_rng(6)
    B, N = 3, 4
    r, rl = dev(rng.integers(0, 3, size=(B, 70))), dev(rng.integers(0, 71, size=B), torch.int32)
    h, hl = dev(rng.integers(0, 3, size=(B, N, 80))), dev(rng.integers(0, 81, size=(B, N)), torch.int32)
    want = ref.batch(r.cpu().numpy(), rl.cpu().numpy(), h.cpu().numpy(), hl.cpu().numpy())
    totals = torch.zeros(8, dtype=torch.int64, device=DEV)
    ops.edit_distance(r, rl, h, hl, totals=totals)                          # eager once (warm-up), then start from zero again
    totals.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dist, counts, _ = ops.edit_distance(r, rl, h, hl, totals=totals)
    totals.zero_()                                                          # whatever the capture itself did does not count
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(totals.cpu().numpy(), 2 * want[2])
    np.testing.assert_array_equal(dist.cpu().numpy(), want[0])
    np.testing.assert_array_equal(counts.cpu().numpy(), want[1])


def test_the_limit_2048():
    """pair_fast is pinned to pair on the CPU (tests/test_edit_distance.py) at sizes where pure Python is quick"""
    rng = np.random.default_rng(7)
    L = ops.EDIT_MAX_LEN
    r = rng.integers(0, 4, size=(2, L))
    h = rng.integers(0, 4, size=(2, 1, L))
    got = check(r, [L, L], h, [[L], [0]], fn=ref.pair_fast)
    assert got[0][1, 0] == L and got[1][1, 0].tolist() == [0, L, 0] and 0 < got[0][0, 0] < L
    check(r[:, :0], [0, 0], h, [[L], [17]], fn=ref.pair_fast)               # an empty reference tensor: all insertions


def test_nbest_at_the_limit_2048():
    """N = 3 at the widest shape: the workgroup's LDS holds one wave's row, so one wave takes the three hypotheses in turn"""
    rng = np.random.default_rng(8)
    L = ops.EDIT_MAX_LEN
    r = rng.integers(0, 4, size=(1, L))
    h = rng.integers(0, 4, size=(1, 3, L))
    h[0, 1, :1500] = r[0, :1500]                                            # one hypothesis nearer than the 1-best: the oracle
    got = check(r, [L], h, [[L, L, 1100]], fn=ref.pair_fast)
    assert got[2][6] == got[0][0, 1] < got[2][2] == got[0][0, 0]


def test_empty_batch():
    totals = torch.arange(8, dtype=torch.int64, device=DEV)
    dist, counts, t = ops.edit_distance(torch.zeros((0, 5), dtype=torch.long, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                        torch.zeros((0, 3, 6), dtype=torch.long, device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                                        totals=totals)
    assert dist.shape == (0, 3) and counts.shape == (0, 3, 3) and t is totals and totals.tolist() == list(range(8))
