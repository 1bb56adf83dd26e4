"""n-gram estimation benchmark (NGramLM.train, csrc/ngramtrain.hip): a seeded Zipf-distributed corpus at AISHELL's size -- 120 k
sentences of 6 .. 22 units (14 on average), V = 4233 -- at order 3 and order 4.  Per order, from device events after a warm-up:
the count pass (otr_ngram_count) with the allocation and zeroing of its table timed apart, the statistics pass (otr_ngram_stats), the
probability passes (otr_ngram_estimate, one launch per order), then on the host the whole NGramLM.train call (passes, downloads,
sorting and the numpy table build), the table build alone (NGramLM._build), and, in the same run, the dict-based restatement of
tests/ngram_train_ref.py on the same corpus (it imports that restatement, so it runs from a checkout with tests/ beside tools/).
Also the number of entries, the count table's load and max_probe.  One probe of contention: the count pass over 120 k EMPTY
sentences, where all 240 k threads add to the same three entries (<s>, </s>, <s> </s>) and nothing else happens.  The times bracket
launches on an otherwise idle stream; they are not kernel times from a profiler.  Prints one JSON line per order.

    python tools/ngram_train_bench.py [--sentences 120000] [--iters 10] [--no-host] [--out f.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import ngram as ng, ops          # noqa: E402
from opentransformer_amd.ngram import NGramLM             # noqa: E402
from tests import ngram_train_ref as ref_impl             # noqa: E402

V, EOS_UNIT = 4233, 1


def make_corpus(n, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(6, 23, size=n)
    T = int(lens.max())
    ids = np.arange(2, V)
    rng.shuffle(ids)                                       # rank -> id: the frequent units are spread over the id range
    tok = ids[np.minimum(rng.zipf(1.2, size=(n, T)), len(ids)) - 1]
    tok[np.arange(T)[None, :] >= lens[:, None]] = 0
    return tok.astype(np.int64), lens.astype(np.int32)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sentences', type=int, default=120000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true', help='skip the host restatement')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ngram_train_bench needs a GPU')
    dev = 'cuda'
    tok, lens = make_corpus(a.sentences)
    d_tok, d_len = torch.from_numpy(tok).to(dev), torch.from_numpy(lens).to(dev)
    sents = [tok[b, :lens[b]].tolist() for b in range(len(lens))]
    empty_tok = torch.zeros((a.sentences, 1), dtype=torch.int64, device=dev)
    empty_len = torch.zeros(a.sentences, dtype=torch.int32, device=dev)
    lines = []
    for order in (3, 4):
        cap = ng.min_capacity(ng.count_bound(lens, order))
        state = {}

        def zero():
            state['t'] = torch.zeros((cap, 4), dtype=torch.int64, device=dev)

        def count():
            state['table'], state['err'] = ops.ngram_train_count(d_tok, d_len, order, V, EOS_UNIT, cap)

        def stats():                                       # on a fresh copy each time: the pass adds into the table
            state['work'].copy_(state['table'])
            state['glob'] = ops.ngram_train_stats(state['work'], order, V, state['err'])

        def copy_only():
            state['work'].copy_(state['table'])

        def estimate():
            ops.ngram_train_estimate(state['work'], order, V, V - 1, state['disc'], state['glob'], state['err'])

        zero_ms = timed(zero, a.iters, a.warmup)
        count_ms = timed(count, a.iters, a.warmup)          # includes the zeroing above
        state['work'] = torch.empty_like(state['table'])
        copy_ms = timed(copy_only, a.iters, a.warmup)
        stats_ms = timed(stats, a.iters, a.warmup)          # includes the copy above
        g = state['glob'].cpu().numpy()
        state['disc'] = [list(ng.kn_discounts(g[4 + 4 * m:8 + 4 * m]) or ng.FALLBACK_DISCOUNTS) for m in range(order)]
        est_ms = timed(estimate, a.iters, a.warmup)
        assert int(state['err'].item()) == 0
        hot_ms = timed(lambda: ops.ngram_train_count(empty_tok, empty_len, order, V, EOS_UNIT, 1024), a.iters, a.warmup)
        hot_zero_ms = timed(lambda: torch.zeros((1024, 4), dtype=torch.int64, device=dev), a.iters, a.warmup)
        train_s = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lm = NGramLM.train(d_tok, d_len, order=order, vocab_size=V, device=dev)
            train_s.append(time.perf_counter() - t0)
        ids, lens_g, logp, backoff = lm.entries()
        lo, hi = ng.pack_keys(ids, lens_g)
        val = np.zeros(len(lo), np.uint64)
        t0 = time.perf_counter()
        NGramLM._build(lo, hi, val, lm.capacity)
        build_s = time.perf_counter() - t0
        rec = {'order': order, 'sentences': a.sentences, 'tokens': int(lens.sum()), 'V': V, 'iters': a.iters,
               'count_table_capacity': cap, 'count_table_mib': cap * 32 >> 20, 'count_load': round(lm.stats['count_load'], 4),
               'entries': lm.stats['entries'], 'ngrams': lm.stats['ngrams'], 'table_capacity': lm.capacity,
               'max_probe': lm.max_probe, 'fallback_orders': lm.stats['fallback_orders'],
               'zero_table_ms': round(zero_ms[0], 3), 'count_ms_with_zero': round(count_ms[0], 3),
               'count_ms': round(count_ms[0] - zero_ms[0], 3), 'stats_ms': round(stats_ms[0] - copy_ms[0], 3),
               'estimate_ms': round(est_ms[0], 3), 'device_passes_ms': round(count_ms[0] + stats_ms[0] - copy_ms[0] + est_ms[0], 3),
               'hot_entries_count_ms': round(hot_ms[0] - hot_zero_ms[0], 3),
               'train_call_s': round(float(np.median(train_s)), 3), 'host_table_build_s': round(build_s, 3),
               'device': torch.cuda.get_device_name(0)}
        if not a.no_host:
            t0 = time.perf_counter()
            est = ref_impl.estimate(sents, order, V)
            rec['host_restatement_s'] = round(time.perf_counter() - t0, 3)
            rec['host_over_device_passes'] = round(rec['host_restatement_s'] * 1e3 / rec['device_passes_ms'], 1)
            rec['host_over_train_call'] = round(rec['host_restatement_s'] / rec['train_call_s'], 1)
            assert len(est['logp']) == lm.stats['entries']
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
