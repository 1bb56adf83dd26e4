"""CPU (-m "not gpu"): WER / CER scoring.  The restatement (tests/edit_distance_ref.py) against hand-checked pairs and against itself by
three routes; the library refuses bad shapes before it launches (no GPU here); the op refuses what it cannot serve; the meter's
arithmetic; the host side of score_texts and tools/compute_wer.py.  Everything is integer: every comparison is exact."""
import ctypes as C
import importlib.util
import math
import os
import random

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, evaluate
from tests import edit_distance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compute_wer():
    spec = importlib.util.spec_from_file_location('compute_wer', os.path.join(ROOT, 'tools', 'compute_wer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_hand_checked_pairs():
    # kitten -> sitting: k/s, e/i substituted and g inserted.  The hypothesis is one token longer than the reference, so I - D = 1:
    # (3 S, 0 D, 0 I) cannot be; the canonical alignment is 2 substitutions and 1 insertion (and the mirror pair 2 S + 1 D).
    assert ref.pair('kitten', 'sitting') == (3, 2, 0, 1)
    assert ref.pair('sitting', 'kitten') == (3, 2, 1, 0)
    assert ref.pair('sunday', 'sundae') == (1, 1, 0, 0)
    for n in (1, 5, 17):
        assert ref.pair([], list(range(n))) == (n, 0, 0, n)
        assert ref.pair(list(range(n)), []) == (n, 0, n, 0)
        assert ref.pair(list(range(n)), list(range(n))) == (0, 0, 0, 0)
    assert ref.pair([], []) == (0, 0, 0, 0)
    for R, H in ((5, 2), (9, 8), (3, 3)):                        # disjoint alphabets, R >= H: H substitutions, R - H deletions
        assert ref.pair(list(range(R)), list(range(100, 100 + H))) == (R, H, R - H, 0)


def test_tie_is_decided_by_the_preference():
    """ref = [a, b], hyp = [b, a]: two substitutions and (delete a, keep b, insert a) both cost 2; the diagonal comes first"""
    for fn in (ref.pair, ref.pair_backtrace, ref.pair_fast):
        assert fn([7, 8], [8, 7]) == (2, 2, 0, 0)
        # above before left: ref = [a, b], hyp = [b]: D[2][1] = 1 by the diagonal (b == b) from D[1][0] = 1 deletion
        assert fn([7, 8], [8]) == (1, 0, 1, 0)
        assert fn([8], [7, 8]) == (1, 0, 0, 1)


def test_three_routes_agree_on_random_pairs():
    rnd = random.Random(0)
    for alphabet in (2, 3, 50):
        for _ in range(1200):
            r = [rnd.randrange(alphabet) for _ in range(rnd.randint(0, 40))]
            h = [rnd.randrange(alphabet) for _ in range(rnd.randint(0, 40))]
            a = ref.pair(r, h)
            assert a == ref.pair_backtrace(r, h) == ref.pair_fast(r, h), (r, h)
            assert a[0] == a[1] + a[2] + a[3] and a[3] - a[2] == len(h) - len(r)


def test_batch_totals_eos_and_validity():
    E = 9
    refs = np.array([[1, 2, 3, 4], [5, 6, 0, 0], [1, 1, 1, 1]])
    ref_len = [4, 2, 3]
    hyp = np.array([[[1, 2, 3, 4], [1, 2, 0, 0]],                # 0 errors; 2 deletions
                    [[5, 7, 6, 8], [5, 6, 3, 3]],                # len 3: 1 insertion; len 2: exact
                    [[1, 1, E, 1], [E, 1, 1, 1]]])               # cut at eos: [1, 1] -> 1 deletion; [] -> 3 deletions
    hyp_len = [[4, 2], [3, 2], [4, 4]]
    dist, counts, totals = ref.batch(refs, ref_len, hyp, hyp_len, eos=E)
    assert dist.tolist() == [[0, 2], [1, 0], [1, 3]]
    assert counts.tolist() == [[[0, 0, 0], [0, 2, 0]], [[0, 0, 1], [0, 0, 0]], [[0, 1, 0], [0, 3, 0]]]
    #                         utterances, ref tokens, errors, S, D, I, oracle (0 + 0 + 1), bad
    assert totals.tolist() == [3, 9, 2, 0, 1, 1, 1, 0]
    # an eos beyond hyp_len is not seen; without eos the token is an ordinary one
    assert ref.batch(refs[2:], [3], np.array([[[1, 1, 1, E]]]), [[3]], eos=E)[0].tolist() == [[0]]
    assert ref.batch(refs[2:], [3], hyp[2:], [[4, 4]], eos=-1)[0].tolist() == [[1, 1]]                        # one insertion each
    assert ref.batch(refs[2:], [3], hyp[2:, 0], None, eos=E)[0].tolist() == [[1]]                       # [B, Lh], the full width
    # invalid lengths: -1 and width + 1.  A bad reference or hypothesis 0 makes the utterance `bad`; a bad hypothesis 1 only leaves the oracle
    dist, counts, totals = ref.batch(refs, [4, -1, 5], hyp, [[4, 2], [3, 2], [4, 4]])
    assert dist.tolist() == [[0, 2], [-1, -1], [-1, -1]] and (counts[1:] == -1).all()
    assert totals.tolist() == [1, 4, 0, 0, 0, 0, 0, 2]
    dist, counts, totals = ref.batch(refs, ref_len, hyp, [[5, 2], [3, -1], [4, 4]])
    assert dist.tolist() == [[-1, 2], [1, -1], [1, 1]] and counts[0, 0].tolist() == [-1, -1, -1] and counts[1, 1].tolist() == [-1, -1, -1]
    assert totals.tolist() == [2, 5, 2, 0, 0, 2, 2, 1]           # utterance 1: the oracle is its 1-best alone; one insertion each


def test_edit_distance_entry_refuses_bad_shapes_without_a_gpu():
    lib = _lib.load()
    al = C.c_void_p(4096)

    def call(B=2, N=3, Lr=10, Lh=10, eos=-1, ref=al, hyp=al, totals=al, ref_bs=10, hyp_bs=30, hyp_ns=10):
        return lib.otr_edit_distance(ref, ref_bs, al, hyp, hyp_bs, hyp_ns, al, B, N, Lr, Lh, eos, al, al, totals, None)
    for kw, word in ((dict(N=0), b'32'), (dict(N=33), b'32'), (dict(Lh=2049), b'2048'), (dict(Lr=2049), b'2048'), (dict(B=-1), b'B='),
                     (dict(eos=-2), b'eos'), (dict(ref=None), b'null'), (dict(hyp=None), b'null'), (dict(totals=None), b'null'),
                     (dict(totals=C.c_void_p(4100)), b'aligned'), (dict(hyp_ns=-1), b'stride')):
        assert call(**kw) < 0, kw
        msg = lib.otr_last_error_string()
        assert b'edit_distance' in msg and word in msg, (kw, msg)
    assert call(B=0) == 0 and call(B=0, ref=None, hyp=None, totals=None) == 0          # nothing to do: no launch


def test_op_refuses_cpu_tensors_and_shapes_over_the_limits():
    from opentransformer_amd import ops
    assert ops.EDIT_MAX_LEN == 2048 and ops.EDIT_MAX_NBEST == 32
    r, rl = torch.ones(2, 4, dtype=torch.long), torch.tensor([4, 4])
    with pytest.raises(_lib.OtransHipError):
        ops.edit_distance(r, rl, torch.ones(2, 3, 4, dtype=torch.long), torch.full((2, 3), 4))
    with pytest.raises(_lib.OtransHipError):
        ops.edit_distance(r, rl, torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match='32'):
        ops.edit_distance(r, rl, torch.ones(2, 33, 4, dtype=torch.long))
    with pytest.raises(ValueError, match='32'):
        ops.edit_distance(r, rl, torch.ones(2, 0, 4, dtype=torch.long))
    with pytest.raises(ValueError, match='2048'):
        ops.edit_distance(r, rl, torch.ones(2, 1, 2049, dtype=torch.long))
    with pytest.raises(ValueError, match='2048'):
        ops.edit_distance(torch.ones(2, 2049, dtype=torch.long), rl, torch.ones(2, 1, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.edit_distance(r, rl, torch.ones(3, 1, 4, dtype=torch.long))


def test_meter_arithmetic():
    m = evaluate.ErrorRateMeter('cpu')
    assert m.totals.dtype == torch.int64 and m.totals.tolist() == [0] * 8
    res = m.result()
    assert math.isnan(res['wer']) and math.isnan(res['topn_wer']) and res['ref_tokens'] == 0 and res['bad'] == 0
    m.totals.copy_(torch.tensor([7, 200, 31, 12, 9, 10, 17, 2]))
    res = m.result()
    assert res == {'wer': 31 / 200 * 100, 'topn_wer': 17 / 200 * 100, 'utterances': 7, 'ref_tokens': 200, 'errors': 31,
                   'substitutions': 12, 'deletions': 9, 'insertions': 10, 'errors_oracle': 17, 'bad': 2}
    m.reset()
    assert m.totals.tolist() == [0] * 8


def test_texts_to_ids_and_compute_wer_parsing(tmp_path):
    refs = {'u1': ['a', 'b', 'a'], 'u2': ['c'], 'u3': []}
    hyps = {'u2': ['d', 'c'], 'x9': ['a'], 'u1': ['a', 'b'], 'u3': []}
    r, rl, h, hl, ids, unmatched = evaluate.texts_to_ids(refs, hyps)
    assert ids == ['u2', 'u1', 'u3'] and unmatched == ['x9']
    assert rl.tolist() == [1, 3, 0] and hl.tolist() == [2, 2, 0] and r.dtype == torch.int64 and rl.dtype == torch.int32
    # equal words share an id, different words do not, and no word has the padding's id
    a, b, c, d = int(r[1, 0]), int(r[1, 1]), int(r[0, 0]), int(h[0, 0])
    assert r[1].tolist() == [a, b, a] and h[1, :2].tolist() == [a, b] and h[0].tolist() == [d, c]
    assert len({a, b, c, d, 0}) == 5
    want = ref.batch(r.numpy(), rl.numpy(), h.numpy(), hl.numpy())
    assert want[2].tolist() == [3, 4, 2, 0, 1, 1, 2, 0]
    lists = evaluate.texts_to_ids([['a'], ['b', 'c']], [['a'], ['c']])
    assert lists[4] == [0, 1] and lists[5] == [] and lists[1].tolist() == [1, 2]
    with pytest.raises(ValueError):
        evaluate.texts_to_ids([['a']], [])
    with pytest.raises(TypeError):
        evaluate.texts_to_ids({'a': []}, [[]])

    cw = _compute_wer()
    tgt, prd = tmp_path / 'target.txt', tmp_path / 'predict.txt'
    tgt.write_text('u1 a b a\nu2 c\n\nu3\n', encoding='utf-8')
    prd.write_text('u2  d c \nu1 a b\nu3\n', encoding='utf-8')
    t, p = cw.read_units(str(tgt)), cw.read_units(str(prd))
    assert t == refs and p == {'u2': ['d', 'c'], 'u1': ['a', 'b'], 'u3': []} and list(p) == ['u2', 'u1', 'u3']
    cw.check_ids(t, p)
    with pytest.raises(KeyError, match='x9'):
        cw.check_ids(t, dict(p, x9=['a']))
    text = cw.report(evaluate.result_from_totals(want[2]))
    assert text.splitlines()[0] == 'The WER/CER is 50.00' and '0 substitutions, 1 deletions, 1 insertions' in text
