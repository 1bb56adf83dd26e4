"""Joint CTC/attention decode benchmark: the C5 shape of tools/decode_bench.py (transformer_baseline dims with a CTC head, batch 8,
beam 10, 4-block TransformerLM shallow fusion, T' 249, max_len 60, EOS suppressed) decoded on the KV-cached loop under hipGraph replay
with and without joint_ctc (ctc_weight 0.3, ctc_beam = int(1.5 * beam) = 15).  Prints one JSON line: ms per decode step of both, their
ratio, and the device time of the new launches alone (otr_joint_prebeam, otr_ctc_prefix_score) at the step's shape.

    python tools/joint_decode_bench.py [--batch 8] [--beam 10] [--max-len 60] [--mode fp16] [--iters 3] [--out FILE]
    python tools/joint_decode_bench.py --profile-once      (one warm joint decode batch, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import synthetic as syn      # noqa: E402


def build(mode, dev, ctc_weight):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import TransformerLanguageModel
    ops.set_compute_dtype(mode)
    model = ota.SpeechToText(syn.c2_model(0.0, ctc_weight=ctc_weight))
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


def kernel_us(fn, iters=50):
    """device time of fn's launches by CUDA events, microseconds per call"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--max-len', type=int, default=60)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--ctc-weight', type=float, default=0.3)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-once', action='store_true')
    args = ap.parse_args(argv)
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    dev = torch.device('cuda:0')
    model, lm = build(args.mode, dev, args.ctc_weight)
    inputs, _ = syn.synthetic_batch(args.batch, args.frames, 80, 4234, 15, seed=0)
    x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
    kw = dict(beam_width=args.beam, nbest=1, max_len=args.max_len, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1,
              idx2unit={i: str(i) for i in range(4234)}, apply_cache=True, ctc_weight=args.ctc_weight)
    if args.profile_once:
        rec = SpeechToTextRecognizer(model, joint_ctc=True, **kw)
        rec.recognize(x, m)                       # warm: captures the step graphs
        torch.cuda.synchronize()
        rec.recognize(x, m)
        torch.cuda.synchronize()
        return None
    with torch.no_grad():
        enc = SpeechToTextRecognizer(model, **kw)
        t_enc, (mem, mmask, _, _) = timed(lambda: enc.encode(x, m), args.iters, args.warmup)
        t_head, _ = timed(lambda: model.assistor.inference(mem, mmask), args.iters, args.warmup)
    res, hyps = {}, {}
    for tag, joint in (('plain', False), ('joint', True)):
        rec = SpeechToTextRecognizer(model, joint_ctc=joint, **kw)
        t, (h, _) = timed(lambda: rec.recognize(x, m), args.iters, args.warmup)
        pre = t_enc + (t_head if joint else 0.0)
        hyps[tag] = [u[0] for u in h]
        res[tag] = {'s_per_batch': t, 'utt_per_s': args.batch / t, 'ms_per_step': (t - pre) * 1e3 / args.max_len,
                    'tokens_per_hyp': len(hyps[tag][0].split())}
    # the new launches alone at the step's shape: R = batch * beam hypotheses, K' candidates, T' frames, a prefix of 30 tokens
    B, beam, K = args.batch, args.beam, int(1.5 * args.beam)
    R = B * beam
    V = 4234
    with torch.no_grad():
        log_probs, length = model.assistor.inference(mem, mmask)
        log_probs, length = log_probs.float().contiguous(), length.to(torch.int32)
    T = log_probs.shape[1]
    g = torch.Generator(device='cpu').manual_seed(0)
    logits = torch.randn(R, V, generator=g).to(dev)
    lm_logits = torch.randn(R, V, generator=g).to(dev)
    preds = torch.randint(2, V, (R, args.max_len + 2), generator=g).to(dev)
    cand_s, cand_i = ops.joint_prebeam(logits, lm_logits, 0.7, 0.1, K, V)
    st = [(torch.zeros(R * K, T, device=dev), torch.zeros(R * K, T, device=dev), torch.zeros(R * K, device=dev)) for _ in range(2)]
    jsrc = torch.arange(R, dtype=torch.int32, device=dev) * K
    k_score = torch.empty(R, beam, device=dev)
    k_idx = torch.empty(R, beam, dtype=torch.long, device=dev)
    k_src = torch.empty(R, beam, dtype=torch.int32, device=dev)

    def prefix(t):
        return lambda: ops.ctc_prefix_score(log_probs, length, cand_i, preds, t, beam, model.assistor.blank, 1, jsrc, st[0], st[1],
                                            cand_score=cand_s, ctc_weight=args.ctc_weight, beam=beam, k_score=k_score, k_idx=k_idx,
                                            k_src=k_src)
    kern = {'joint_prebeam_us': kernel_us(lambda: ops.joint_prebeam(logits, lm_logits, 0.7, 0.1, K, V, cand_s, cand_i)),
            'ctc_prefix_score_us': kernel_us(prefix(31)),
            'ctc_prefix_score_first_step_us': kernel_us(prefix(1))}
    out = {'metric': 'joint CTC/attention decode: ms per cached + hipGraph step (C5: beam %d + TransformerLM fusion, ctc_weight %.2f, '
                     'ctc_beam %d, T\' %d, max_len %d)' % (args.beam, args.ctc_weight, K, T, args.max_len),
           'value': res['joint']['ms_per_step'], 'unit': 'ms/step', 'dtype': args.mode, 'batch': args.batch,
           'plain_ms_per_step': res['plain']['ms_per_step'], 'ratio_joint_over_plain': res['joint']['ms_per_step'] / res['plain']['ms_per_step'],
           'target_ratio': 1.25, 'encode_ms': t_enc * 1e3, 'ctc_head_ms': t_head * 1e3, 'loops': res, 'kernels': kern,
           'iters': args.iters, 'warmup': args.warmup}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out) + '\n')
    return out


if __name__ == '__main__':
    main()
