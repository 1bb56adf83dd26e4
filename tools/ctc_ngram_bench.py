"""LM-fused CTC prefix beam search benchmark (CTCRecognizer mode='beam', ngram_lm=...): the shape of tools/ctc_beam_bench.py, batch
32 x T' 250 x V 4233, beam 10, cutoff_top_n 40, on peaky random log-probs, with a synthetic order-3 table of about 2 M n-grams
(64 MB of entries in a 128 MB table: the probes leave the L2).  In one run it times otr_ctc_beam_search and
otr_ctc_beam_search_lm on the same top-K buffers with device events, medians of --iters, in --blocks alternating blocks whose
spread is reported; --parent-lib times otr_ctc_beam_search of another build of the library (the parent commit's) in the same
blocks, which shows what the template split cost the plain search.  Prints one JSON line.

    python tools/ctc_ngram_bench.py [--ngrams 2000000] [--iters 50] [--blocks 3] [--parent-lib old/libotrans_hip.so] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L      # noqa: E402
from opentransformer_amd.ngram import NGramLM  # noqa: E402


def synthetic_lm(V, n, seed=0):
    """every unigram, then random 2-grams and 3-grams (distinct by construction of the draw + the table's own dedup), n in all"""
    rng = np.random.default_rng(seed)
    n2 = (n - V - 1) // 2
    n3 = n - V - 1 - n2
    ids = np.zeros((n, 3), np.int64)
    lens = np.ones(n, np.int64)
    ids[:V + 1, 0] = np.arange(V + 1)
    ids[V + 1:V + 1 + n2, :2] = rng.integers(1, V, size=(n2, 2))
    ids[V + 1:V + 1 + n2 // 8, 0] = V                                  # some start at <s>
    lens[V + 1:V + 1 + n2] = 2
    ids[V + 1 + n2:] = rng.integers(1, V, size=(n3, 3))
    lens[V + 1 + n2:] = 3
    lp = -rng.uniform(0.2, 7.0, size=n).astype(np.float32)
    bo = -rng.uniform(0.0, 2.0, size=n).astype(np.float32)
    return NGramLM(3, V, ids, lens, lp, bo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--topk', type=int, default=40)
    ap.add_argument('--ngrams', type=int, default=2000000)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='libotrans_hip.so of the parent commit: its otr_ctc_beam_search is timed too')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_ngram_bench needs a GPU')
    dev = 'cuda'
    B, T, V, W, K = a.batch, a.frames, a.vocab, a.beam, a.topk
    rng = np.random.default_rng(0)
    lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * 4.0), -1).to(dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    lm = synthetic_lm(V, a.ngrams)
    table = lm.device_table(dev)
    lib = L.load()
    parent = C.CDLL(a.parent_lib) if a.parent_lib else None
    top_lp = torch.empty((B * T, K), dtype=torch.float32, device=dev)
    top_tok = torch.empty((B * T, K), dtype=torch.int32, device=dev)
    ws_bytes = lib.otr_ctc_beam_workspace_bytes(B, T, W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    outs = {k: (torch.empty((B, W, T), dtype=torch.int64, device=dev), torch.empty((B, W), dtype=torch.int32, device=dev),
                torch.empty((B, W), dtype=torch.float32, device=dev)) for k in ('plain', 'lm', 'parent')}
    lm_scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    L.check(lib.otr_ctc_topk(p(lp), V, p(ln), B, T, V, K, p(top_lp), p(top_tok), stream()), 'otr_ctc_topk')

    def plain(which=lib, key='plain'):
        tk, ol, sc = outs[key]
        rc = which.otr_ctc_beam_search(p(top_lp), p(top_tok), p(ln), C.c_int32(B), C.c_int32(T), C.c_int32(V), C.c_int32(K),
                                       C.c_int32(0), C.c_int32(W), p(ws), C.c_int64(ws_bytes), p(tk), p(ol), p(sc), stream())
        if rc < 0:
            raise RuntimeError('otr_ctc_beam_search (%s) refused the call' % key)

    def fused():
        tk, ol, sc = outs['lm']
        L.check(lib.otr_ctc_beam_search_lm(p(top_lp), p(top_tok), p(ln), B, T, V, K, 0, W, p(ws), ws_bytes, p(tk), p(ol), p(sc),
                                           p(table), lm.capacity, lm.max_probe, lm.order, a.alpha, a.beta, lm.oov_score,
                                           p(lm_scores), stream()), 'otr_ctc_beam_search_lm')

    runs = [('plain', plain), ('lm', fused)] + ([('parent', lambda: plain(parent, 'parent'))] if parent else [])
    for _ in range(a.warmup):
        for _, f in runs:
            f()
    torch.cuda.synchronize()
    med = {k: [] for k, _ in runs}
    for _ in range(a.blocks):
        for k, f in runs:
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            med[k].append(float(np.median(ts)))
    best = lambda k: float(np.median(med[k]))              # noqa: E731
    res = {
        'batch': B, 'frames': T, 'vocab': V, 'beam': W, 'topk': K, 'iters': a.iters, 'blocks': a.blocks,
        'lm_order': lm.order, 'lm_entries': lm.stats['entries'], 'lm_capacity': lm.capacity, 'lm_table_MB': lm.capacity * 32 >> 20,
        'lm_max_probe': lm.max_probe, 'alpha': a.alpha, 'beta': a.beta,
        'search_ms_median': round(best('plain'), 4), 'search_ms_blocks': [round(v, 4) for v in med['plain']],
        'search_lm_ms_median': round(best('lm'), 4), 'search_lm_ms_blocks': [round(v, 4) for v in med['lm']],
        'lm_over_plain': round(best('lm') / best('plain'), 3),
        'search_us_per_frame': round(best('plain') * 1e3 / T, 3), 'search_lm_us_per_frame': round(best('lm') * 1e3 / T, 3),
        'mean_1best_len': round(float(outs['lm'][1][:, 0].float().mean()), 1),
        'one_best_changed_by_lm': '%d/%d' % (sum(not torch.equal(outs['lm'][0][b, 0], outs['plain'][0][b, 0]) for b in range(B)), B),
        'device': torch.cuda.get_device_name(0),
    }
    if parent:
        res.update(parent_search_ms_median=round(best('parent'), 4), parent_search_ms_blocks=[round(v, 4) for v in med['parent']],
                   plain_over_parent=round(best('plain') / best('parent'), 4),
                   parent_equal_outputs=all(torch.equal(x, y) for x, y in zip(outs['plain'], outs['parent'])))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
