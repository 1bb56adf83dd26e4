"""C5 decode benchmark: batch beam search, beam 10, TransformerLM shallow fusion (4 blocks),
transformer_baseline dims, T=1000 frames, max_len 60, EOS suppressed so every hypothesis runs all 60 steps
(random-init weights would stop at step 1).  Prints one JSON line: utterances/s and ms per decode step for the
reference-style re-forward loop, the KV-cached loop (eager launches) and the KV-cached loop under hipGraph replay,
plus `roofline` (bytes one cached step must stream / step time / 8 TB/s) and the CPU oracle on a bounded sample.

    python tools/decode_bench.py [--batch 8] [--beam 10] [--max-len 60] [--mode fp16] [--no-cpu-baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import synthetic as syn      # noqa: E402


def build(mode, dev):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import TransformerLanguageModel
    ops.set_compute_dtype(mode)
    model = ota.SpeechToText(syn.c2_model(0.0))
    syn.fill_state_dict_(model.state_dict(), 1234)
    lm = TransformerLanguageModel(syn.lm_config(4234))
    syn.fill_state_dict_(lm.state_dict(), 4321)
    with torch.no_grad():
        model.decoder.output_layer.bias[1] = -30.0
    return model.to(dev).eval(), lm.to(dev).eval()


def timed(fn, iters, warmup=1):
    for _ in range(max(1, warmup)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters, out


def main(argv=None, emit=True, outputs=None):
    """outputs: a dict that receives what the last timed call of the hipGraph loop returned -- 'hyps' [batch, nbest, max_len]
    (token ids as float32, -1 past the end) and 'scores' [batch, nbest] (float64)"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--max-len', type=int, default=60)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args(argv)
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    dev = torch.device('cuda:0')
    model, lm = build(args.mode, dev)
    inputs, _ = syn.synthetic_batch(args.batch, args.frames, 80, 4234, 15, seed=0)
    x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
    idx2unit = {i: str(i) for i in range(4234)}
    kw = dict(beam_width=args.beam, nbest=1, max_len=args.max_len, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1,
              idx2unit=idx2unit)
    res = {}
    hyps = {}
    with torch.no_grad():
        enc = SpeechToTextRecognizer(model, **kw)
        t_enc, _ = timed(lambda: enc.encode(x, m), args.iters, args.warmup)
    for tag, cache, graph in (('reforward', False, False), ('cached_eager', True, False), ('cached_hipgraph', True, True)):
        rec = SpeechToTextRecognizer(model, apply_cache=cache, **kw)
        rec.use_hipgraph = graph
        t, (h, s) = timed(lambda: rec.recognize(x, m), args.iters, args.warmup)
        hyps[tag] = [u[0] for u in h]
        res[tag] = {'s_per_batch': t, 'utt_per_s': args.batch / t,
                    'ms_per_step': (t - t_enc) * 1e3 / args.max_len}
        if tag == 'cached_hipgraph' and outputs is not None:
            unit2idx = {u: i for i, u in idx2unit.items()}
            ids = np.full((len(h), max(len(u) for u in h), args.max_len), -1.0, dtype=np.float32)
            for b, nb in enumerate(h):
                for k, hyp in enumerate(nb):
                    tok = [unit2idx[u] for u in hyp.split()]
                    ids[b, k, :len(tok)] = tok
            outputs.update(hyps=ids, scores=torch.as_tensor(s).double().cpu().numpy())
    same = sum(a == b for a, b in zip(hyps['reforward'], hyps['cached_hipgraph']))
    out = {'metric': 'decode utterances/sec (C5: beam %d + TransformerLM fusion, max_len %d, %d frames)'
                     % (args.beam, args.max_len, args.frames),
           'value': res['cached_hipgraph']['utt_per_s'], 'unit': 'utterances/s', 'dtype': args.mode,
           'batch': args.batch, 'encode_ms': t_enc * 1e3, 'loops': res,
           'speedup_vs_reforward': res['reforward']['s_per_batch'] / res['cached_hipgraph']['s_per_batch'],
           'identical_1best': '%d/%d' % (same, args.batch),
           'tokens_per_hyp': len(hyps['cached_hipgraph'][0].split())}
    # roofline of the cached step: it is a weight stream -- every decoder + LM weight (16-bit shadows) and the cross-attention
    # keys / values of the batch are read once per step for ~0.4 GFLOP of work -- so the bound is HBM bandwidth
    esz = 4 if args.mode == 'fp32' else 2
    wbytes = sum(p.numel() for p in model.decoder.parameters()) * esz + sum(p.numel() for p in lm.parameters()) * esz
    Tm = ((args.frames - 3) // 2 + 1 - 3) // 2 + 1
    kv_bytes = args.batch * Tm * 2 * 256 * esz * len(model.decoder.blocks)
    step_s = res['cached_hipgraph']['ms_per_step'] * 1e-3
    ach = (wbytes + kv_bytes) / step_s / 1e9
    out['roofline'] = {'bound': 'hbm', 'kernel': 'one KV-cached decode step (decoder + LM: 34 launches under one hipGraph, 23 on the decoder chain; r04: ~140)',
                       'note': 'a chain of dependent launches over <= 80 workgroups: the bound that binds is the launch chain (DESIGN.md 5.7), the HBM figure is the weight stream once per step',
                       'achieved': ach, 'peak': 8000.0, 'unit': 'GB/s', 'frac': ach / 8000.0, 'traffic': None,
                       'algorithmic_bytes': wbytes + kv_bytes, 'avg_launch_ms': res['cached_hipgraph']['ms_per_step']}
    if not args.no_cpu_baseline:
        from oracle import otrans_oracle as orc
        from tests import helpers as H
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        cfg = syn.c2_model(0.0)
        parts = H.filled_state(cfg)
        parts['decoder']['output_layer.bias'][1] = -30.0
        lm_cfg = syn.lm_config(4234)
        lmp = H.lm_state(lm_cfg)
        nb, ml = 1, min(args.max_len, 12)
        t0 = time.perf_counter()
        orc.beam_search(parts, cfg, inputs['inputs'][:nb], inputs['mask'][:nb], beam=args.beam, nbest=1, max_len=ml,
                        penalty=0.6, lamda=5, lm=(lmp, lm_cfg), lm_weight=0.1)
        dt = time.perf_counter() - t0
        out['cpu_baseline'] = {'value': nb / dt, 'unit': 'utterances/s at max_len %d' % ml, 's_per_utt_at_max_len_%d' % ml: dt / nb,
                               'cores': torch.get_num_threads(), 'host_cores': os.cpu_count(), 'kind': 'port',
                               'sample': 'CPU oracle beam search (re-forward, like the reference), %d utterance, '
                                         'max_len %d' % (nb, ml)}
    # the driver's contract keys (bench.py --task decode): a step = one batch of utterances decoded end to end
    out.update(n_gpus=1, steps=args.iters, warmup=args.warmup, ms_per_step=res['cached_hipgraph']['s_per_batch'] * 1e3,
               higher_is_better=True, scaling='weak', vs_baseline=None, data='synthetic',
               config={'workload': 'C5: transformer_baseline dims (12 enc / 6 dec), batch %d x %d frames, beam %d, 4-block TransformerLM '
                                   'shallow fusion (weight 0.1), max_len %d, EOS suppressed; KV-cached decoder step replayed as one hipGraph'
                                   % (args.batch, args.frames, args.beam, args.max_len), 'global_batch': args.batch})
    if emit:
        print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
