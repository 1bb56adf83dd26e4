"""Phrase biasing in the attention and joint decoders (SpeechToTextRecognizer bias=...): the C5 decode shape with a CTC head
(transformer_baseline dims, batch 32, beam 10, 4-block TransformerLM shallow fusion, T' 249, max_len 60, EOS suppressed, fp16,
KV-cached loop under hipGraph replay) with 1000 random phrases of 2-8 units.  In one run it times one decode STEP of the plain and
the joint search with and without the phrases: every step of a 50-step decode between two device events, the median of the 50, in
--blocks alternating blocks whose spread is reported.  --parent-lib times the bias=None steps of another build of the library (the
parent commit's) in the same blocks, and both builds TWICE (two recognizers each, two pairs of graphs, captured in the order this
build, parent, this build, parent): the bias=None step issues the launches it issued before, so the ratio to the parent says what
this change cost the decode that does not use it, and the ratios between the two runs of one build say how much of that is the
measurement.  Also the new launches alone at the step's shape (50 of them as the nodes of one graph): on random prefixes, and on
prefixes that stand inside a phrase, where the walk is as long as the phrase.  Prints one JSON line.

    python tools/bias_bench.py [--batch 32] [--iters 50] [--blocks 3] [--parent-lib DIR_OR_SO] [--out f.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L              # noqa: E402
from opentransformer_amd import synthetic as syn       # noqa: E402
from opentransformer_amd.bias import PhraseBias        # noqa: E402
from tools.ngram_attn_bench import V, Step, build, foreign_lib, kernel_us      # noqa: E402


def random_phrases(n, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(2, V, size=rng.integers(2, 9))] for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--max-len', type=int, default=60)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--phrases', type=int, default=1000)
    ap.add_argument('--score', type=float, default=2.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--parent-lib', default=None, help='the parent commit\'s library (a .so of the --mode build, or the directory '
                                                       'holding both builds): its bias=None steps are timed in the same blocks, twice')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bias_bench needs a GPU')
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    dev = torch.device('cuda:0')
    model, lm = build(a.mode, dev)
    kind = 'fp16' if a.mode == 'fp16' else 'bf16'
    inputs, _ = syn.synthetic_batch(a.batch, a.frames, 80, V, 15, seed=0)
    x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
    pb = PhraseBias(random_phrases(a.phrases), V, score=a.score).to(dev)
    kw = dict(beam_width=a.beam, nbest=1, max_len=a.max_len, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, ctc_weight=0.3,
              idx2unit={i: str(i) for i in range(V)})
    steps = {}
    for tag, joint, with_bias in (('plain', False, False), ('plain_bias', False, True), ('joint', True, False), ('joint_bias', True, True)):
        steps[tag] = Step(SpeechToTextRecognizer(model, apply_cache=True, joint_ctc=joint, bias=pb if with_bias else None, **kw), x, m)
    if a.parent_lib:                                        # parent, this build again, parent again: two runs of each
        ours = L.load(kind)
        for again in ('', '_again'):
            L._libs[kind] = foreign_lib(a.parent_lib, kind)     # the parent's kernels go into the graphs captured now
            try:
                for tag, joint in (('parent_plain', False), ('parent_joint', True)):
                    steps[tag + again] = Step(SpeechToTextRecognizer(model, apply_cache=True, joint_ctc=joint, **kw), x, m)
            finally:
                L._libs[kind] = ours
            if not again:
                for tag, joint in (('plain_again', False), ('joint_again', True)):
                    steps[tag] = Step(SpeechToTextRecognizer(model, apply_cache=True, joint_ctc=joint, **kw), x, m)
    med = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, s in steps.items():
            med[k].append(s.block(a.iters))
    best = lambda k: float(np.median(med[k]))              # noqa: E731
    spread = lambda k: (max(med[k]) - min(med[k])) / best(k)     # noqa: E731
    res = {'metric': 'phrase biasing in the cached decode step: ms per hipGraph step (C5 with a CTC head, batch %d, beam %d, '
                     'TransformerLM, T\' %d, %s)' % (a.batch, a.beam, steps['plain'].mem.shape[1], a.mode),
           'batch': a.batch, 'beam': a.beam, 'bias_beam': min(V, int(1.5 * a.beam)), 'max_len': a.max_len, 'dtype': a.mode,
           'iters': a.iters, 'blocks': a.blocks, 'phrases': len(pb.phrases), 'nodes': pb.n_nodes, 'table_KB': pb.capacity * 16 >> 10,
           'max_probe': pb.max_probe,
           'step_ms_median': {k: round(best(k), 4) for k in steps}, 'step_ms_blocks': {k: [round(v, 4) for v in med[k]] for k in steps},
           'block_spread': {k: round(spread(k), 4) for k in steps},
           'plain_bias_over_plain': round(best('plain_bias') / best('plain'), 4),
           'plain_bias_minus_plain_us': round((best('plain_bias') - best('plain')) * 1e3, 2),
           'joint_bias_over_joint': round(best('joint_bias') / best('joint'), 4),
           'joint_bias_minus_joint_us': round((best('joint_bias') - best('joint')) * 1e3, 2),
           'device': torch.cuda.get_device_name(0)}
    if a.parent_lib:
        res.update(plain_over_parent=round(best('plain') / best('parent_plain'), 4),
                   plain_again_over_parent=round(best('plain_again') / best('parent_plain'), 4),
                   parent_plain_again_over_parent=round(best('parent_plain_again') / best('parent_plain'), 4),
                   joint_again_over_parent=round(best('joint_again') / best('parent_joint'), 4),
                   joint_over_parent=round(best('joint') / best('parent_joint'), 4),
                   parent_joint_again_over_parent=round(best('parent_joint_again') / best('parent_joint'), 4))
    # the new launches alone at the step's shape: R = batch * beam rows, K' candidates, prefixes of 30 tokens
    R, K = a.batch * a.beam, min(V, int(1.5 * a.beam))
    g = torch.Generator(device='cpu').manual_seed(0)
    preds = torch.randint(2, V, (R, a.max_len + 2), generator=g).to(dev)
    cand_s, cand_i = ops.joint_prebeam(torch.randn(R, V, generator=g).to(dev), None, 1.0, 0.0, K, V)
    k_score = torch.empty(R, a.beam, device=dev)
    k_idx = torch.empty(R, a.beam, dtype=torch.long, device=dev)
    out = torch.empty_like(cand_s)
    hyp = torch.randint(2, V, (R, 249), generator=g).to(dev)
    hyp_len = torch.randint(10, 31, (R,), generator=g).to(torch.int32).to(dev)
    # rows that stand inside a phrase: the chain is deep, the walk is the phrase's length
    inside = preds.clone()
    for r in range(R):
        p = pb.phrases[r % len(pb.phrases)]
        inside[r, 31 - (len(p) - 1):31] = torch.tensor(p[:-1])
    res['kernels_us'] = {
        'bias_score_cands_select': round(kernel_us(lambda: ops.bias_score_candidates(
            pb, preds, cand_i, cand_s, 1, t=31, beam=a.beam, cand_out=out, k_score=k_score, k_idx=k_idx)), 2),
        'bias_score_cands_add_only': round(kernel_us(lambda: ops.bias_score_candidates(pb, preds, cand_i, cand_s, 1, t=31, cand_out=out)), 2),
        'bias_score_cands_select_inside_phrases': round(kernel_us(lambda: ops.bias_score_candidates(
            pb, inside, cand_i, cand_s, 1, t=31, beam=a.beam, cand_out=out, k_score=k_score, k_idx=k_idx)), 2),
        'bias_score_seqs': round(kernel_us(lambda: ops.bias_score_sequences(pb, hyp, hyp_len)), 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
