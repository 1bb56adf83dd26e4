"""n-gram LM fusion in the attention, joint and two-pass decoders (SpeechToTextRecognizer ngram_lm=...): the C5 decode shape with a
CTC head (transformer_baseline dims, batch 32, beam 10, 4-block TransformerLM shallow fusion, T' 249, max_len 60, EOS suppressed,
fp16, KV-cached loop under hipGraph replay) with the synthetic order-3 table of tools/ctc_ngram_bench.py (about 1.86 M entries,
128 MB: the probes leave the L2).  In one run it times one decode STEP of the plain and the joint search with and without the
n-gram: every step of a 50-step decode between two device events, the median of the 50, in --blocks alternating blocks whose spread
is reported.  --parent-lib times the no-n-gram steps of another build of the library (the parent commit's) in the same blocks: the
same launches, so the ratio says what this change cost the decode that does not use it.  Also the two-pass decode (rescore=True)
with and without the n-gram, and the new launches alone at the step's shape (50 of them as the nodes of one graph).  Prints one JSON line.

    python tools/ngram_attn_bench.py [--batch 32] [--iters 50] [--blocks 3] [--parent-lib DIR_OR_SO] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L              # noqa: E402
from opentransformer_amd import synthetic as syn       # noqa: E402
from tools.ctc_ngram_bench import synthetic_lm         # noqa: E402

V = 4234


def build(mode, dev):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import TransformerLanguageModel
    ops.set_compute_dtype(mode)
    model = ota.SpeechToText(syn.c2_model(0.0, ctc_weight=0.3))
    syn.fill_state_dict_(model.state_dict(), 1234)
    lm = TransformerLanguageModel(syn.lm_config(V))
    syn.fill_state_dict_(lm.state_dict(), 4321)
    with torch.no_grad():
        model.decoder.output_layer.bias[1] = -30.0
    return model.to(dev).eval(), lm.to(dev).eval()


def foreign_lib(path, kind):
    """another build of the library behind this binding's signatures (no ABI check: only entries both builds have are called)"""
    if os.path.isdir(path):
        path = os.path.join(path, os.path.basename(L.LIB_PATHS[kind]))
    lib = C.CDLL(path)
    for name, argtypes in L.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = argtypes, L._RESTYPE.get(name, C.c_int32)
    return lib


class Step:
    """one recognizer whose cached state has captured its two step graphs; block() decodes `iters` steps from a fresh start and
    returns the median device time of a step in ms"""

    def __init__(self, rec, x, m):
        self.rec = rec
        with torch.no_grad():
            rec.recognize(x, m)                            # eager visits, then the captures
            rec.recognize(x, m)
            self.mem, self.mm, _, _ = rec.encode(x, m)
            self.head = rec._ctc_head(self.mem, self.mm) if rec.joint_ctc else None
        self.st = next(iter(rec._cached_states.values()))
        assert all(g is not None for g in self.st.graphs)
        torch.cuda.synchronize()

    def block(self, iters):
        st = self.st
        assert iters <= self.rec.max_len
        with torch.no_grad():
            st.load_memory(self.mem, self.mm)
            if st.joint is not None:
                st.joint.load(*self.head)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        cur = 0
        ev[0].record()
        for i in range(iters):
            st._launch(cur)
            cur ^= 1
            ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]))


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def kernel_us(fn, iters=50):
    """device time of fn's launches as nodes of one captured graph (host launch time out of the picture; the graph's launch boundary,
    which a decode step pays as well, in it), microseconds per call, the median of five replays"""
    from opentransformer_amd import ops
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return event_ms(g.replay, 5) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--max-len', type=int, default=60)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--ngrams', type=int, default=2000000)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--parent-lib', default=None, help='the parent commit\'s library (a .so of the --mode build, or the directory '
                                                       'holding both builds): its no-n-gram steps are timed in the same blocks')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ngram_attn_bench needs a GPU')
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    dev = torch.device('cuda:0')
    model, lm = build(a.mode, dev)
    kind = 'fp16' if a.mode == 'fp16' else 'bf16'
    inputs, _ = syn.synthetic_batch(a.batch, a.frames, 80, V, 15, seed=0)
    x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
    ng = synthetic_lm(V, a.ngrams).to(dev)
    kw = dict(beam_width=a.beam, nbest=1, max_len=a.max_len, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, ctc_weight=0.3,
              idx2unit={i: str(i) for i in range(V)})
    ngkw = dict(ngram_lm=ng, alpha=a.alpha, beta=a.beta)
    steps = {}
    for tag, joint, with_ng in (('plain', False, False), ('plain_ngram', False, True), ('joint', True, False), ('joint_ngram', True, True)):
        steps[tag] = Step(SpeechToTextRecognizer(model, apply_cache=True, joint_ctc=joint, **(ngkw if with_ng else {}), **kw), x, m)
    if a.parent_lib:
        ours = L.load(kind)
        L._libs[kind] = foreign_lib(a.parent_lib, kind)     # the parent's kernels go into the graphs captured now
        try:
            for tag, joint in (('parent_plain', False), ('parent_joint', True)):
                steps[tag] = Step(SpeechToTextRecognizer(model, apply_cache=True, joint_ctc=joint, **kw), x, m)
        finally:
            L._libs[kind] = ours
    med = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, s in steps.items():
            med[k].append(s.block(a.iters))
    best = lambda k: float(np.median(med[k]))              # noqa: E731
    spread = lambda k: (max(med[k]) - min(med[k])) / best(k)     # noqa: E731
    res = {'metric': 'n-gram LM fusion in the cached decode step: ms per hipGraph step (C5 with a CTC head, batch %d, beam %d, '
                     'TransformerLM, T\' %d, %s)' % (a.batch, a.beam, steps['plain'].mem.shape[1], a.mode),
           'batch': a.batch, 'beam': a.beam, 'ngram_beam': min(V, int(1.5 * a.beam)), 'max_len': a.max_len, 'dtype': a.mode,
           'iters': a.iters, 'blocks': a.blocks, 'alpha': a.alpha, 'beta': a.beta,
           'lm_order': ng.order, 'lm_entries': ng.stats['entries'], 'lm_table_MB': ng.capacity * 32 >> 20, 'lm_max_probe': ng.max_probe,
           'step_ms_median': {k: round(best(k), 4) for k in steps}, 'step_ms_blocks': {k: [round(v, 4) for v in med[k]] for k in steps},
           'block_spread': {k: round(spread(k), 4) for k in steps},
           'plain_ngram_over_plain': round(best('plain_ngram') / best('plain'), 4),
           'plain_ngram_minus_plain_us': round((best('plain_ngram') - best('plain')) * 1e3, 2),
           'joint_ngram_over_joint': round(best('joint_ngram') / best('joint'), 4),
           'joint_ngram_minus_joint_us': round((best('joint_ngram') - best('joint')) * 1e3, 2),
           'device': torch.cuda.get_device_name(0)}
    if a.parent_lib:
        res.update(plain_over_parent=round(best('plain') / best('parent_plain'), 4),
                   joint_over_parent=round(best('joint') / best('parent_joint'), 4))
    # the two-pass decode behind the CTC head, with and without the n-gram
    with torch.no_grad():
        mem, mm = steps['joint'].mem, steps['joint'].mm
        log_probs, length = model.assistor.inference(mem, mm)
        log_probs = log_probs.float().contiguous()
        two = {}
        for tag, extra in (('rescore', {}), ('rescore_ngram', ngkw)):
            rec = SpeechToTextRecognizer(model, rescore=True, **extra, **dict(kw, max_len=32))
            for _ in range(3):
                rec.rescore_pass(mem, mm, log_probs, length)
            two[tag] = [event_ms(lambda: rec.rescore_pass(mem, mm, log_probs, length), a.iters) for _ in range(a.blocks)]
    res.update(rescore_pass_ms_blocks={k: [round(v, 4) for v in two[k]] for k in two},
               rescore_pass_ms_median={k: round(float(np.median(two[k])), 4) for k in two},
               rescore_ngram_over_rescore=round(float(np.median(two['rescore_ngram']) / np.median(two['rescore'])), 4))
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
    res['kernels_us'] = {
        'ngram_score_cands_select': round(kernel_us(lambda: ops.ngram_score_candidates(
            ng, preds, cand_i, cand_s, a.alpha, a.beta, 1, t=31, beam=a.beam, cand_out=out, k_score=k_score, k_idx=k_idx)), 2),
        'ngram_score_cands_add_only': round(kernel_us(lambda: ops.ngram_score_candidates(
            ng, preds, cand_i, cand_s, a.alpha, a.beta, 1, t=31, cand_out=out)), 2),
        'ngram_score_seqs': round(kernel_us(lambda: ops.ngram_score_sequences(ng, hyp, hyp_len, a.alpha, a.beta)), 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
