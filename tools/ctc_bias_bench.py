"""Phrase-biased CTC prefix beam search benchmark (CTCRecognizer mode='beam', bias=...; the first pass of SpeechToTextRecognizer
rescore=True, bias_first_pass=True): the shape of tools/ctc_ngram_bench.py, batch 32 x T' 250 x V 4233, beam 10, cutoff_top_n 40, on
peaky random log-probs, with 1000 random phrases of 2-8 units (the recipe of tools/bias_bench.py) and that tool's synthetic order-3
n-gram table.  In one run, in --blocks alternating blocks whose spread is reported, device events around the search launch only,
medians of --iters: the search plain (otr_ctc_beam_search), with phrases, with the n-gram (otr_ctc_beam_search_lm), with both
(otr_ctc_beam_search_bias), and with phrases on frames that spell phrase prefixes, so that every slot stands inside a match (deep
chains).  --parent-lib times the plain and the n-gram search of another build of the library (the parent commit's) in the same
blocks, twice, next to a second run of this build's: the parent's own second-run spread is the margin the comparison has.
Prints one JSON line.

    python tools/ctc_bias_bench.py [--phrases 1000] [--iters 50] [--blocks 3] [--parent-lib old/libotrans_hip.so] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L          # noqa: E402
from opentransformer_amd.bias import PhraseBias    # noqa: E402
from tools.ctc_ngram_bench import synthetic_lm     # noqa: E402


def random_phrases(n, V, seed=0):
    """tools/bias_bench.py's recipe over V units"""
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(2, V, size=rng.integers(2, 9))] for _ in range(n)]


def inside_phrases(phrases, B, T, V, seed=1):
    """log-probs whose frames spell phrases without their last unit, one after the other (unit, blank, unit, blank ...): the best
    hypotheses stand inside a match at nearly every frame"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, T, V)).astype(np.float32) * 4.0
    for b in range(B):
        label = []
        while len(label) < T:
            p = phrases[int(rng.integers(len(phrases)))]
            for u in p[:-1]:
                label += [u, 0]
        for t in range(T):
            x[b, t, label[t]] += 24.0
    return torch.log_softmax(torch.from_numpy(x), -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--topk', type=int, default=40)
    ap.add_argument('--phrases', type=int, default=1000)
    ap.add_argument('--score', type=float, default=2.0)
    ap.add_argument('--ngrams', type=int, default=2000000)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='libotrans_hip.so of the parent commit: its plain and n-gram searches are timed too')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_bias_bench needs a GPU')
    dev = 'cuda'
    B, T, V, W, K = a.batch, a.frames, a.vocab, a.beam, a.topk
    rng = np.random.default_rng(0)
    lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * 4.0), -1).to(dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    pb = PhraseBias(random_phrases(a.phrases, V), V, score=a.score)
    lp_in = inside_phrases(pb.phrases, B, T, V).to(dev)
    bias_table = pb.device_table(dev)
    lm = synthetic_lm(V, a.ngrams)
    table = lm.device_table(dev)
    lib = L.load()
    parent = C.CDLL(a.parent_lib) if a.parent_lib else None
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    tops = {}
    for key, x in (('random', lp), ('inside', lp_in)):
        tops[key] = (torch.empty((B * T, K), dtype=torch.float32, device=dev), torch.empty((B * T, K), dtype=torch.int32, device=dev))
        L.check(lib.otr_ctc_topk(p(x), V, p(ln), B, T, V, K, p(tops[key][0]), p(tops[key][1]), stream()), 'otr_ctc_topk')
    ws_bytes = lib.otr_ctc_beam_workspace_bytes(B, T, W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    outs = {}

    def out(key):
        if key not in outs:
            outs[key] = (torch.empty((B, W, T), dtype=torch.int64, device=dev), torch.empty((B, W), dtype=torch.int32, device=dev),
                         torch.empty((B, W), dtype=torch.float32, device=dev), torch.empty((B, W), dtype=torch.float32, device=dev),
                         torch.empty((B, W), dtype=torch.float32, device=dev))
        return outs[key]

    def plain(which, key):
        tk, ol, sc, _, _ = out(key)
        top_lp, top_tok = tops['random']
        rc = which.otr_ctc_beam_search(p(top_lp), p(top_tok), p(ln), C.c_int32(B), C.c_int32(T), C.c_int32(V), C.c_int32(K),
                                       C.c_int32(0), C.c_int32(W), p(ws), C.c_int64(ws_bytes), p(tk), p(ol), p(sc), stream())
        if rc < 0:
            raise RuntimeError('otr_ctc_beam_search (%s) refused the call' % key)

    def with_lm(which, key):
        tk, ol, sc, ls, _ = out(key)
        top_lp, top_tok = tops['random']
        rc = which.otr_ctc_beam_search_lm(p(top_lp), p(top_tok), p(ln), C.c_int32(B), C.c_int32(T), C.c_int32(V), C.c_int32(K),
                                          C.c_int32(0), C.c_int32(W), p(ws), C.c_int64(ws_bytes), p(tk), p(ol), p(sc), p(table),
                                          C.c_int64(lm.capacity), C.c_int32(lm.max_probe), C.c_int32(lm.order), C.c_float(a.alpha),
                                          C.c_float(a.beta), C.c_float(lm.oov_score), p(ls), stream())
        if rc < 0:
            raise RuntimeError('otr_ctc_beam_search_lm (%s) refused the call' % key)

    def biased(key, top='random', ngram=False):
        tk, ol, sc, ls, bs = out(key)
        top_lp, top_tok = tops[top]
        ng = (p(table), lm.capacity, lm.max_probe, lm.order, a.alpha, a.beta, lm.oov_score, p(ls)) if ngram \
            else (None, 0, 0, 0, 0.0, 0.0, 0.0, None)
        L.check(lib.otr_ctc_beam_search_bias(p(top_lp), p(top_tok), p(ln), B, T, V, K, 0, W, p(ws), ws_bytes, p(tk), p(ol), p(sc), *ng,
                                             p(bias_table), pb.capacity, pb.max_probe, pb.max_len, p(bs), stream()),
                'otr_ctc_beam_search_bias')

    runs = [('plain', lambda: plain(lib, 'plain')), ('bias', lambda: biased('bias')), ('lm', lambda: with_lm(lib, 'lm')),
            ('lm_bias', lambda: biased('lm_bias', ngram=True)), ('bias_inside_phrases', lambda: biased('bias_inside_phrases', 'inside'))]
    if parent:                                              # parent, this build again, parent again: two runs of each
        runs += [('parent_plain', lambda: plain(parent, 'parent_plain')), ('parent_lm', lambda: with_lm(parent, 'parent_lm')),
                 ('plain_again', lambda: plain(lib, 'plain')), ('lm_again', lambda: with_lm(lib, 'lm')),
                 ('parent_plain_again', lambda: plain(parent, 'parent_plain')), ('parent_lm_again', lambda: with_lm(parent, 'parent_lm'))]
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
    spread = lambda k: (max(med[k]) - min(med[k])) / best(k)     # noqa: E731
    depth = lambda key: round(float(outs[key][4][:, 0].mean()), 2)      # noqa: E731
    res = {
        'metric': 'CTC prefix beam search: ms per search launch (events around the launch only)',
        'batch': B, 'frames': T, 'vocab': V, 'beam': W, 'topk': K, 'iters': a.iters, 'blocks': a.blocks,
        'phrases': len(pb.phrases), 'nodes': pb.n_nodes, 'bias_table_KB': pb.capacity * 16 >> 10, 'bias_max_probe': pb.max_probe,
        'bias_max_len': pb.max_len, 'score': a.score,
        'lm_order': lm.order, 'lm_entries': lm.stats['entries'], 'lm_table_MB': lm.capacity * 32 >> 20, 'alpha': a.alpha, 'beta': a.beta,
        'search_ms_median': {k: round(best(k), 4) for k, _ in runs},
        'search_ms_blocks': {k: [round(v, 4) for v in med[k]] for k, _ in runs},
        'block_spread': {k: round(spread(k), 4) for k, _ in runs},
        'us_per_frame': {k: round(best(k) * 1e3 / T, 3) for k, _ in runs},
        'bias_over_plain': round(best('bias') / best('plain'), 4),
        'bias_inside_phrases_over_plain': round(best('bias_inside_phrases') / best('plain'), 4),
        'lm_over_plain': round(best('lm') / best('plain'), 4),
        'lm_bias_over_plain': round(best('lm_bias') / best('plain'), 4),
        'lm_bias_over_lm': round(best('lm_bias') / best('lm'), 4),
        'mean_1best_bias_score': {k: depth(k) for k in ('bias', 'lm_bias', 'bias_inside_phrases')},
        'one_best_changed_by_phrases': '%d/%d' % (sum(not torch.equal(outs['bias'][0][b, 0], outs['plain'][0][b, 0]) for b in range(B)), B),
        'device': torch.cuda.get_device_name(0),
    }
    if parent:
        res.update(plain_over_parent=round(best('plain') / best('parent_plain'), 4),
                   plain_again_over_parent=round(best('plain_again') / best('parent_plain'), 4),
                   parent_plain_again_over_parent=round(best('parent_plain_again') / best('parent_plain'), 4),
                   lm_over_parent=round(best('lm') / best('parent_lm'), 4),
                   lm_again_over_parent=round(best('lm_again') / best('parent_lm'), 4),
                   parent_lm_again_over_parent=round(best('parent_lm_again') / best('parent_lm'), 4),
                   parent_equal_outputs=all(torch.equal(x, y) for k in ('plain', 'lm')
                                            for x, y in zip(outs[k][:4 if k == 'lm' else 3], outs['parent_' + k])))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
