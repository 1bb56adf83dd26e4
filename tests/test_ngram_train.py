"""CPU (-m "not gpu"): the n-gram estimator behind NGramLM.train.  The dict-based restatement tests/ngram_train_ref.py against a
corpus worked by hand and against the sum-to-one property; NGramLM.to_arpa / from_arpa round trips; the argument refusals of the new
C entries and of NGramLM.train, none of which needs a GPU."""
import ctypes as C
import gzip
import io
import math

import numpy as np
import pytest

from opentransformer_amd import _lib
from opentransformer_amd import ngram as ng
from opentransformer_amd.ngram import NGramLM
from tests import ngram_train_ref as R
from tests.test_ngram import HAND_ARPA, HAND_UNITS

S, E, A, B_ = 4, 1, 2, 3                 # V = 4: <s> is id 4, </s> is unit 1
HAND = [[A, B_], [A], [A, B_]]           # <s> a b </s> / <s> a </s> / <s> a b </s>


def test_restatement_on_a_corpus_worked_by_hand():
    est = R.estimate(HAND, 2, 4)
    assert est['counts'] == {(S,): 3, (A,): 3, (B_,): 2, (E,): 3, (S, A): 3, (A, B_): 2, (B_, E): 2, (A, E): 1}
    # adjusted unigram counts are continuation counts: a follows {<s>}, b follows {a}, </s> follows {a, b} -> 1, 1, 2; the empty
    # context has sum 4, n1 2, n2 1.  Count-of-counts: order 1 (2, 1, 0, 0), order 2 (1, 2, 1, 0): both orders fall back
    assert est['contexts'][()] == [4, 2, 1, 0] and est['contexts'][(A,)] == [3, 1, 1, 0] and est['contexts'][(S,)] == [3, 0, 0, 1]
    assert est['fallback_orders'] == [1, 2] and est['discounts'] == [(0.5, 1.0, 1.5)] * 2
    # gamma(empty) = (0.5 * 2 + 1 * 1) / 4 = 1/2, p0 = 1/3
    want = {(A,): 0.5 / 4 + 0.5 / 3, (B_,): 0.5 / 4 + 0.5 / 3, (E,): 1.0 / 4 + 0.5 / 3,
            (S, A): 1.5 / 3 + 0.5 * (0.5 / 4 + 0.5 / 3),            # gamma(<s>) = 1.5 * 1 / 3
            (A, B_): 1.0 / 3 + 0.5 * (0.5 / 4 + 0.5 / 3),           # gamma(a) = (0.5 + 1) / 3
            (A, E): 0.5 / 3 + 0.5 * (1.0 / 4 + 0.5 / 3),
            (B_, E): 1.0 / 2 + 0.5 * (1.0 / 4 + 0.5 / 3)}           # gamma(b) = 1 * 1 / 2
    assert set(est['logp']) == set(want) | {(S,)}
    for g, p in want.items():
        assert abs(float(est['logp'][g]) - math.log(p)) < 1e-6, g
    assert est['logp'][(S,)] == np.float32(-99 * math.log(10))
    for g in ((S,), (A,), (B_,)):
        assert abs(float(est['backoff'][g]) - math.log(0.5)) < 1e-7
    assert est['backoff'][(E,)] == 0 and est['backoff'][(A, B_)] == 0
    # a unit without a count gets gamma(empty) / |U|; with V = 5 unit 4 is unseen and |U| = 4
    est5 = R.estimate(HAND, 2, 5)
    assert abs(float(est5['logp'][(4,)]) - math.log(0.5 / 4)) < 1e-6 and est5['backoff'][(4,)] == 0
    # the discount formula on count-of-counts worked by hand: Y = 4 / 8; D = 1 - 2 Y 2/4, 2 - 3 Y 1/2, 3 - 4 Y 1/1
    assert ng.kn_discounts([4, 2, 1, 1]) == (0.5, 1.25, 1.0)
    assert ng.kn_discounts([4, 2, 0, 1]) is None and ng.kn_discounts([1, 2, 40, 1]) is None       # a zero; D_2 < 0


@pytest.mark.parametrize('seed,V,order,n,max_len,zipf', [(0, 3, 1, 5, 3, None), (1, 4, 2, 20, 5, None), (2, 4, 4, 30, 6, None),
                                                         (3, 10, 3, 200, 8, 1.5), (4, 50, 4, 400, 12, None), (5, 50, 3, 3000, 10, 1.5),
                                                         (6, 8, 4, 2000, 10, None)])
def test_restatement_sums_to_one(seed, V, order, n, max_len, zipf):
    est = R.estimate(R.random_corpus(seed, n, V, max_len, zipf=zipf), order, V)
    contexts = {g[:-1] for g in est['counts']} | {g for g in est['counts'] if len(g) < order}
    worst = 0.0
    for h in contexts:
        if h and h[-1] == E:
            continue                                  # nothing follows </s>
        worst = max(worst, abs(sum(math.exp(float(R.cond_logp(est, order, h, w))) for w in range(1, V)) - 1.0))
    print('worst |sum - 1| = %.3g over %d contexts' % (worst, len(contexts)))
    assert worst <= 1e-5


def _same_model(a, b):
    return (np.array_equal(a.table, b.table) and a.max_probe == b.max_probe and a.order == b.order and a.vocab_size == b.vocab_size)


def test_to_arpa_round_trip_is_bit_identical(tmp_path):
    units = {i: 'u%d' % i for i in range(50)}
    est = R.estimate(R.random_corpus(3, 300, 50, 9), 4, 50)
    lm = NGramLM(4, 50, *R.arrays(est, 4))
    buf = io.StringIO()
    lm.to_arpa(buf, units)
    text = buf.getvalue()
    assert '\n-99\t<s>\t' in text and '\\data\\' in text and text.rstrip().endswith('\\end\\')
    assert 'ngram 1=%d\n' % sum(len(g) == 1 for g in est['logp']) in text
    assert _same_model(lm, NGramLM.from_arpa(io.StringIO(text), units, capacity=lm.capacity))
    big = NGramLM(4, 50, *R.arrays(est, 4), capacity=4 * lm.capacity)             # another capacity: the same file
    buf2 = io.StringIO()
    big.to_arpa(buf2, units)
    assert buf2.getvalue() == text
    p, z = tmp_path / 'lm.arpa', tmp_path / 'lm.arpa.gz'
    lm.to_arpa(str(p), units)
    lm.to_arpa(z, units)
    assert p.read_text() == text and gzip.open(z, 'rt').read() == text and open(z, 'rb').read(2) == b'\x1f\x8b'
    assert _same_model(lm, NGramLM.from_arpa(z, units, capacity=lm.capacity))
    # a model that from_arpa read (the hand-written fixture, <unk> mapped to a unit): the keys are decoded from the table
    hand = NGramLM.from_arpa(io.StringIO(HAND_ARPA), HAND_UNITS, unk_unit=4)
    buf3 = io.StringIO()
    hand.to_arpa(buf3, HAND_UNITS)
    assert '-99\t<s>\t' in buf3.getvalue() and '\t<s> a b\n' in buf3.getvalue()
    assert _same_model(hand, NGramLM.from_arpa(io.StringIO(buf3.getvalue()), HAND_UNITS, capacity=hand.capacity))
    with pytest.raises(ValueError):
        hand.to_arpa(io.StringIO(), {0: '_', 1: 'e'})                             # names for another vocabulary


def test_new_c_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(4096)

    def count(tokens=p, ld=8, lengths=p, n=4, max_len=8, order=3, V=50, eos=1, table=p, cap=64, err=p):
        return lib.otr_ngram_count(tokens, ld, lengths, n, max_len, order, V, eos, table, cap, err, None)

    def stats(table=p, cap=64, order=3, V=50, glob=p, err=p):
        return lib.otr_ngram_stats(table, cap, order, V, glob, err, None)

    disc = (C.c_double * 12)(*([0.5, 1.0, 1.5] * 4))

    def est(table=p, cap=64, order=3, V=50, n_units=49, d=disc, glob=p, prob=p, logp=p, bo=p, err=p):
        return lib.otr_ngram_estimate(table, cap, order, V, n_units, d, glob, prob, logp, bo, err, None)

    for fn, name in ((count, b'ngram_count'), (stats, b'ngram_stats'), (est, b'ngram_estimate')):
        for kw in (dict(table=None), dict(err=None), dict(order=0), dict(order=5), dict(V=0), dict(V=8193), dict(cap=1), dict(cap=0),
                   dict(cap=48), dict(cap=-64), dict(cap=1 << 32)):
            assert fn(**kw) < 0, (name, kw)
            assert name in lib.otr_last_error_string(), (name, kw)
    assert count(tokens=None) < 0 and count(lengths=None) < 0 and count(n=-1) < 0 and count(max_len=-1) < 0 and count(ld=7) < 0
    assert count(eos=0) < 0 and count(eos=50) < 0
    assert count(n=0, tokens=None, lengths=None) == 0                              # nothing to do
    assert stats(glob=None) < 0 and stats(glob=C.c_void_p(4100)) < 0
    assert est(d=None) < 0 and est(glob=None) < 0 and est(prob=None) < 0 and est(logp=None) < 0 and est(bo=None) < 0
    assert est(n_units=0) < 0 and est(n_units=50) < 0
    assert est(d=(C.c_double * 12)(*([0.5, 2.5, 1.5] * 4))) < 0 and b'discount' in lib.otr_last_error_string()
    assert est(d=(C.c_double * 12)(*([-0.1, 1.0, 1.5] * 4))) < 0


def test_train_refuses_before_any_launch():
    good = [[2, 3], [4]]
    with pytest.raises(ValueError, match='empty corpus'):
        NGramLM.train([], vocab_size=10)
    with pytest.raises(ValueError, match='order 5'):
        NGramLM.train(good, order=5, vocab_size=10)
    with pytest.raises(ValueError):
        NGramLM.train(good, order=0, vocab_size=10)
    for bad in ([[2, 0]], [[10]], [[2, 1, 3]], [[-3]]):                            # PAD, <s>, </s> inside, negative
        with pytest.raises(ValueError, match='ids inside'):
            NGramLM.train(bad, vocab_size=10)
    with pytest.raises(ValueError):
        NGramLM.train(good, vocab_size=8193)
    with pytest.raises(ValueError):
        NGramLM.train(good, vocab_size=10, table_capacity=48)
    with pytest.raises(ValueError):
        NGramLM.train(good, vocab_size=10, units=[2, 3, 4])                        # </s> is not predictable
    with pytest.raises(ValueError):
        NGramLM.train(good, vocab_size=10, discounts=[[0.5, 1.0, 1.5]] * 2)        # order 3 wants three rows
    with pytest.raises(ValueError):
        NGramLM.train(good, order=1, vocab_size=10, discounts=[[1.5, 1.0, 1.5]])   # D_1 > 1
    import torch
    with pytest.raises(ValueError):
        NGramLM.train(torch.zeros((2, 3), dtype=torch.int32), vocab_size=10)       # int64 wanted
    with pytest.raises(ValueError):
        NGramLM.train(torch.ones((2, 3), dtype=torch.int64) * 2, [1, 4], vocab_size=10)   # a length past L
    assert ng.count_bound([0, 1, 5], 3) == (1 + 2) + (1 + 2 + 3) + (1 + 2 + 3 * 5)
    if not torch.cuda.is_available():                                             # no CPU path
        with pytest.raises(_lib.OtransHipError):
            NGramLM.train(good, vocab_size=10)
