"""GPU: NGramLM.train (csrc/ngramtrain.hip) against the dict-based restatement tests/ngram_train_ref.py.  Counts are integers and
compared exactly; log-probs and backoffs are float64 arithmetic on identical integers rounded to f32 once on both sides and compared
to 2 units in the last place (one ulp can differ through `log`, the second is margin).  Shapes are small: what matters is where the
kernel can go wrong -- orders 1 .. 4, sentences shorter than the order, the top of the 16-bit id field, every thread on the same
entries, a probe chain that wraps past the end of the table, a full table."""
import functools
import importlib.util
import io
import math
import os

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from opentransformer_amd import ngram as ng
from opentransformer_amd.ngram import NGramLM
from tests import ngram_train_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = [[], [2], [2, 3], [3, 2, 3], []]                   # lengths 0, 1 and below every order > 1


@functools.lru_cache(maxsize=None)
def corpus(name):
    if name == 'top':                                      # V = 8192: id 8191 and <s> = 8192 = 0x2000 in every key field
        return 8192, [[8191, 2, 8191, 8191], [8191], [], [4097, 8191, 255, 256, 8191], [8191, 8191, 8191, 8191, 8191]]
    if name == 'copies':                                   # every thread of a position contends for the same handful of entries
        return 50, [[3, 2, 3, 2, 5, 49]] * 4096
    if name == 'wrap':                                     # 251 distinct n-grams at order 3: capacity 256, chains wrap
        return 10, R.random_corpus(10, 70, 10, 6)
    kind, V = name
    if kind == 'small':
        return V, SHORT + R.random_corpus(V, 60, V, 7)
    if kind == 'mixed':                                    # computed discounts on orders 2 and 3, the fallback on 1 and 4
        return V, R.random_corpus(3, 500, V, 10)
    if kind == 'zipf':
        return V, SHORT + R.random_corpus(5, 600, V, 10, zipf=1.5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, order, discounts=None):
    V, sents = corpus(name)
    return R.estimate(sents, order, V, discounts=discounts)


def continuation(counts, order):
    """{gram: number of distinct (m+1)-grams that end in it} for the grams below the highest order"""
    out = {g: 0 for g in counts if len(g) < order}
    for g in counts:
        if len(g) > 1:
            out[g[1:]] += 1
    return out


def device_counts(sents, order, V, **kw):
    ids, lens, raw, cont = ng.count_ngrams(sents, order=order, vocab_size=V, device=DEV, **kw)
    grams = [tuple(int(v) for v in r[:m]) for r, m in zip(ids, lens)]
    assert len(set(grams)) == len(grams)
    return dict(zip(grams, raw.tolist())), dict(zip(grams, cont.tolist()))


def check_counts(name, order, **kw):
    V, sents = corpus(name)
    want = reference(name, order)['counts']
    raw, cont = device_counts(sents, order, V, **kw)
    assert raw == want
    wc = continuation(want, order)
    assert {g: c for g, c in cont.items() if len(g) < order} == wc
    return want


def ulps(a, b):
    """distance of two f32 arrays in units in the last place (equal signs or zeros assumed, as for log-probs)"""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def check_values(lm, est, order):
    ids, lens, logp, backoff = lm.entries()
    grams = [tuple(int(v) for v in r[:m]) for r, m in zip(ids, lens)]
    assert sorted(grams) == sorted(est['logp'])
    wl = np.array([est['logp'][g] for g in grams], np.float32)
    wb = np.array([est['backoff'][g] for g in grams], np.float32)
    dl, db = ulps(logp, wl), ulps(backoff, wb)
    print('n-grams %d: worst ulp distance log-prob %d, backoff %d' % (len(grams), dl.max(), db.max()))
    assert dl.max() <= 2 and db.max() <= 2
    assert ((backoff == 0) == (wb == 0)).all()


@pytest.mark.parametrize('order', [1, 2, 3, 4])
@pytest.mark.parametrize('V', [4, 50])
def test_counts_equal_the_restatement(order, V):
    want = check_counts(('small', V), order)
    assert (V,) in want and (V, 1) in want or order == 1     # the empty sentence: <s> </s>


def test_counts_at_the_top_of_the_id_field():
    want = check_counts('top', 4)
    assert (8192, 8191, 8191, 8191) in want and (8191, 8191, 8191, 8191) in want and (4097, 8191, 255, 256) in want


def test_counts_when_every_thread_meets_the_same_entries():
    want = check_counts('copies', 4)
    assert want[(3, 2)] == 2 * 4096 and want[(50, 3, 2, 3)] == 4096
    lm = NGramLM.train(corpus('copies')[1], order=4, vocab_size=50, device=DEV)
    check_values(lm, reference('copies', 4), 4)


def test_counts_with_a_probe_chain_that_wraps():
    V, sents = corpus('wrap')
    want = reference('wrap', 3)['counts']
    cap = 2
    while cap < len(want):
        cap *= 2
    grams = sorted(want)
    ids = np.zeros((len(grams), 3), np.int64)
    for r, g in enumerate(grams):
        ids[r, :len(g)] = g
    lo, hi = ng.pack_keys(ids, [len(g) for g in grams])
    assert (hi == (np.array([len(g) for g in grams], np.uint64) << np.uint64(16))).all()
    home = (ng._hash(lo, hi) & np.uint64(cap - 1)).astype(np.int64)
    full, wrapped = np.zeros(cap, bool), 0
    for h in home:                     # linear probing: which entries end up taken, and how many keys cross the end, does not
        p = h                          # depend on the order of insertion
        while full[p]:
            p = (p + 1) % cap
        full[p] = True
        wrapped += p < h
    assert cap == 256 and len(want) > 0.95 * cap and wrapped >= 1, (cap, len(want), wrapped)
    check_counts('wrap', 3, table_capacity=cap)
    a = NGramLM.train(sents, order=3, vocab_size=V, table_capacity=cap, device=DEV)
    b = NGramLM.train(sents, order=3, vocab_size=V, device=DEV)
    assert np.array_equal(a.table, b.table) and a.stats['count_load'] > 0.95 > b.stats['count_load']
    check_values(a, reference('wrap', 3), 3)


def test_padding_is_never_read():
    V, sents = corpus(('small', 50))
    n, T = len(sents), max(len(s) for s in sents)
    lens = torch.tensor([len(s) for s in sents], dtype=torch.int32)
    clean = torch.zeros((n, T), dtype=torch.int64)
    for b, s in enumerate(sents):
        clean[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    junk = torch.tensor([0, V, 8193, 70000, -1, -(1 << 40), 1, 1 << 33], dtype=torch.int64)
    dirty = junk[torch.arange(n * T).reshape(n, T) % len(junk)]
    mask = torch.arange(T)[None, :] < lens[:, None]
    dirty[mask] = clean[mask]
    wide = junk[torch.arange(2 * n * (T + 5)).reshape(2 * n, T + 5) % len(junk)].to(DEV)
    wide[::2, 2:T + 2] = dirty.to(DEV)
    view = wide[::2, 2:T + 2]                               # rows 2 (T + 5) apart, starting 2 ids into each
    assert not view.is_contiguous() and view.stride(0) == 2 * (T + 5)
    kw = dict(order=3, vocab_size=V, device=DEV)
    base = NGramLM.train(sents, **kw)
    for form in (clean, clean.to(DEV), dirty, dirty.to(DEV), view):
        for ln in (lens, lens.to(DEV), lens.tolist()):
            lm = NGramLM.train(form, ln, **kw)
            assert np.array_equal(lm.table, base.table) and lm.max_probe == base.max_probe and lm.stats['ngrams'] == base.stats['ngrams']
    check_values(base, reference(('small', 50), 3), 3)
    with pytest.raises(ValueError):                          # the same junk inside a length: the kernel's error word
        NGramLM.train(dirty.to(DEV), (lens + 1).clamp(max=T).to(DEV), **kw)
    assert np.array_equal(NGramLM.train(view, lens, **kw).table, base.table)        # and the process goes on


@pytest.mark.parametrize('name,order', [(('mixed', 50), 4), (('zipf', 50), 3), (('small', 4), 4), (('small', 50), 1), ('top', 4)])
def test_values_equal_the_restatement(name, order):
    V, sents = corpus(name)
    est = reference(name, order)
    lm = NGramLM.train(sents, order=order, vocab_size=V, device=DEV)
    if name == ('mixed', 50):
        assert est['fallback_orders'] == [1, 4]             # orders 2 and 3 on computed discounts, 1 and 4 on the fallback
    assert lm.stats['fallback_orders'] == est['fallback_orders']
    assert np.allclose(np.array(lm.stats['discounts']), np.array(est['discounts']), rtol=1e-14, atol=0)
    assert lm.stats['sentences'] == len(sents) and lm.stats['tokens'] == sum(len(s) for s in sents)
    assert lm.stats['ngrams'] == [sum(len(g) == m for g in est['logp']) for m in range(1, order + 1)]
    check_values(lm, est, order)


def test_values_with_explicit_discounts_and_units():
    D = ((0.3, 0.9, 1.2), (0.7, 1.1, 2.5), (0.9, 1.9, 2.9))
    V, sents = corpus(('zipf', 50))
    est = reference(('zipf', 50), 3, D)
    lm = NGramLM.train(sents, order=3, vocab_size=V, discounts=D, device=DEV)
    assert lm.stats['fallback_orders'] == [] and lm.stats['discounts'] == [tuple(d) for d in D]
    check_values(lm, est, 3)
    seen = sorted({w for s in sents for w in s} | {1})
    est_u = R.estimate(sents, 3, V, units=seen + [48] if 48 not in seen else seen)
    lm_u = NGramLM.train(sents, order=3, vocab_size=V, units=seen + [48] if 48 not in seen else seen, device=DEV)
    check_values(lm_u, est_u, 3)
    with pytest.raises(ValueError):
        NGramLM.train(sents, order=3, vocab_size=V, units=seen[:-1], device=DEV)     # a unit of the corpus left out


@pytest.mark.parametrize('order', [3, 4])
def test_trained_model_sums_to_one_on_the_device(order):
    V = 20
    sents = SHORT + R.random_corpus(order, 300, V, 8)
    lm = NGramLM.train(sents, order=order, vocab_size=V, device=DEV)
    ids, lens, _, _ = lm.entries()
    contexts = {()} | {tuple(int(v) for v in r[:m]) for r, m in zip(ids, lens) if m < order and r[m - 1] != 1}
    contexts = sorted(contexts)
    ctxs = [h for h in contexts for _ in range(1, V)]
    toks = [w for _ in contexts for w in range(1, V)]
    got = lm.lookup(ctxs, toks, device=DEV).cpu().numpy()
    host = lm.lookup_host(ctxs, toks)
    assert (got > lm.oov_score).all()                        # every unit is predictable: none scores oov_score
    assert (np.abs(got - host) <= 1e-6 * np.abs(host) + 1e-6).all()
    tot = np.exp(got.astype(np.float64)).reshape(len(contexts), V - 1).sum(1)
    print('order %d: %d contexts, worst |sum - 1| = %.3g' % (order, len(contexts), np.abs(tot - 1).max()))
    assert np.abs(tot - 1).max() <= 1e-5


def test_result_does_not_depend_on_order():
    V, sents = corpus(('zipf', 50))
    perm = np.random.default_rng(0).permutation(len(sents))
    a = NGramLM.train(sents, order=4, vocab_size=V, device=DEV)
    b = NGramLM.train(sents, order=4, vocab_size=V, device=DEV)
    c = NGramLM.train([sents[i] for i in perm], order=4, vocab_size=V, device=DEV)
    for o in (b, c):
        assert np.array_equal(a.table, o.table) and a.max_probe == o.max_probe and a.stats['ngrams'] == o.stats['ngrams']


def test_full_count_table_is_refused():
    V, sents = corpus('wrap')                                # 251 distinct n-grams
    with pytest.raises(_lib.OtransHipError, match='count table is full'):
        NGramLM.train(sents, order=3, vocab_size=V, table_capacity=128, device=DEV)
    with pytest.raises(_lib.OtransHipError, match='count table is full'):
        ng.count_ngrams(sents, order=3, vocab_size=V, table_capacity=2, device=DEV)
    lm = NGramLM.train(SHORT, order=2, vocab_size=4, device=DEV)                      # the process stays usable
    check_values(lm, R.estimate(SHORT, 2, 4), 2)


def test_train_ngram_tool_end_to_end(tmp_path):
    spec = importlib.util.spec_from_file_location('train_ngram', os.path.join(ROOT, 'tools', 'train_ngram.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    units = ['<PAD>', '<S/E>', '<UNK>'] + list('abcdefgh')
    vocab = tmp_path / 'vocab'
    vocab.write_text(''.join('%s %d\n' % (u, i) for i, u in enumerate(units)), encoding='utf-8')
    V = len(units)
    sents = [s for s in R.random_corpus(8, 120, V, 9) if s] + [[2, 3, 2]]
    text = tmp_path / 'text'
    lines = ['utt%d %s' % (k, ' '.join('zz' if w == 2 else units[w] for w in s)) for k, s in enumerate(sents)]
    text.write_text('\n'.join(lines + ['', 'bad a <S/E> b', 'empty']) + '\n', encoding='utf-8')
    out = tmp_path / 'lm.arpa.gz'
    lm, rep = tool.train_file(str(text), str(vocab), str(out), order=3)
    sents = sents + [[]]                                     # the line with an id and no unit is an empty sentence
    assert rep['skipped'] == 1 and rep['unk'] == sum(w == 2 for s in sents for w in s) and rep['sentences'] == len(sents)
    direct = NGramLM.train(sents, order=3, vocab_size=V, device=DEV)
    idx2unit = dict(enumerate(units))
    back = NGramLM.from_arpa(str(out), idx2unit, capacity=direct.capacity)
    assert np.array_equal(back.table, direct.table) and np.array_equal(lm.table, direct.table)
    bare = tmp_path / 'bare'
    bare.write_text('\n'.join(line.split(' ', 1)[1] if ' ' in line else '' for line in lines) + '\n', encoding='utf-8')
    lm2, _ = tool.train_file(str(bare), str(vocab), str(tmp_path / 'lm2.arpa'), order=3, ids=False)
    assert lm2.stats['sentences'] == len(sents) - 1          # no id, no unit: no sentence
    est = R.estimate(sents, 3, V)
    T = max(len(s) for s in sents)
    tok = torch.full((len(sents), T), -1, dtype=torch.int64)
    for b, s in enumerate(sents):
        tok[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    got = back.score(tok.to(DEV), torch.tensor([len(s) for s in sents], dtype=torch.int32, device=DEV)).cpu().numpy()
    want = np.array([R.sentence_logp(est, 3, V, s) for s in sents])
    assert np.isfinite(got).all() and (np.abs(got - want) <= 1e-4 * np.abs(want)).all()
