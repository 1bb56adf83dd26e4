"""Two-pass decode benchmark: the C5 shape of tools/joint_decode_bench.py (transformer_baseline dims with a CTC head, T' 249, 4-block
TransformerLM, fp16) decoded by SpeechToTextRecognizer(rescore=True) -- CTC prefix beam search (W 10, K 40), then ONE teacher-forced
pass of the decoder and the LM over all B x W hypotheses -- beside the unchanged KV-cached attention beam search (apply_cache=True,
beam 10, max_len 60, EOS suppressed) on the same inputs.  Per batch size, device time by events: encoder + CTC head, the search, and
the second pass split into pack / decoder + output layer / LM / score + select; wall-clock utterances/s of both decodes.

The synthetic model's CTC head is flat: quiet_blank() makes it peaky and raises the blank's bias until about --tokens (default 18)
frames per utterance prefer a non-blank, so the hypotheses have the 15-20 tokens of real transcripts and fit max_len.

    python tools/rescore_decode_bench.py [--batches 8,32] [--beam 10] [--max-len 32] [--mode fp16] [--iters 5] [--out FILE]
    python tools/rescore_decode_bench.py --profile-once      (one warm two-pass batch of 32, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
from opentransformer_amd import synthetic as syn      # noqa: E402
from joint_decode_bench import build, timed            # noqa: E402


def event_ms(fn, iters, warmup=2):
    """device time of fn's launches by events, ms per call"""
    for _ in range(warmup):
        out = fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, out


def quiet_blank(model, mem, n_tokens):
    """make the synthetic CTC head behave like a trained one: peaky (its logits scaled to a standard deviation of 8, so one token
    dominates a frame) and mostly blank (the blank's bias raised until about n_tokens frames per utterance prefer a non-blank)"""
    with torch.no_grad():
        out = model.assistor.output_layer
        gain = 8.0 / float(model.assistor.compute_logits(mem).float().std())
        out.weight *= gain
        out.bias *= gain
        lg = model.assistor.compute_logits(mem).float()
        margin = lg[..., 0] - lg[..., 1:].max(-1).values                  # blank over the best non-blank, per frame
        out.bias[0] -= torch.quantile(margin.flatten(), min(1.0, n_tokens / margin.shape[1]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='8,32')
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--cutoff', type=int, default=40)
    ap.add_argument('--max-len', type=int, default=32)
    ap.add_argument('--plain-max-len', type=int, default=60)
    ap.add_argument('--tokens', type=int, default=18)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--ctc-weight', type=float, default=0.3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-once', action='store_true')
    args = ap.parse_args(argv)
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import BOS, EOS, SpeechToTextRecognizer, _output
    dev = torch.device('cuda:0')
    model, lm = build(args.mode, dev, args.ctc_weight)
    V, W = 4234, args.beam
    common = dict(beam_width=W, nbest=1, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, idx2unit={i: str(i) for i in range(V)},
                  ctc_weight=args.ctc_weight)
    res, tuned = {}, False
    for B in ([32] if args.profile_once else [int(b) for b in args.batches.split(',')]):
        inputs, _ = syn.synthetic_batch(B, args.frames, 80, V, 15, seed=0)
        x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
        rec = SpeechToTextRecognizer(model, rescore=True, cutoff_top_n=args.cutoff, max_len=args.max_len, **common)
        with torch.no_grad():
            mem, mm, _, _ = rec.encode(x, m)
            if not tuned:
                quiet_blank(model, mem, args.tokens)
                tuned = True
        if args.profile_once:
            rec.recognize(x, m)
            torch.cuda.synchronize()
            rec.recognize(x, m)
            torch.cuda.synchronize()
            return None
        dec = model.decoder
        with torch.no_grad():
            head = lambda: model.assistor.inference(*rec.encode(x, m)[:2])                     # noqa: E731
            t_head, (lp, ln) = event_ms(head, args.iters)
            lp = lp.float().contiguous()
            search = lambda: ops.ctc_prefix_beam_search(lp, ln, beam_width=W, cutoff_top_n=args.cutoff, blank=0)    # noqa: E731
            t_search, (tokens, out_len, scores) = event_ms(search, args.iters)
            t_pack, packed = event_ms(lambda: ops.rescore_pack(tokens, out_len, scores, args.max_len, V, BOS, EOS), args.iters)
            out_dec, out_lm = rec._rescore_outputs()
            t_dec, logits = event_ms(lambda: _output(out_dec, dec.output_layer, dec.hidden(packed[0], mem, mm, share=W)), args.iters)
            t_lm, lm_logits = event_ms(lambda: _output(out_lm, lm.output_project, lm.hidden(packed[0])), args.iters)
            t_sel, out = event_ms(lambda: ops.attention_rescore(logits, tokens, out_len, scores, args.max_len, V, args.ctc_weight,
                                                                lm_logits=lm_logits, lm_weight=0.1, nbest=1, penalty=0.6, lamda=5,
                                                                packed=packed), args.iters)
            t_pass, _ = event_ms(lambda: rec.rescore_pass(mem, mm, lp, ln), args.iters)
            t_two, _ = timed(lambda: rec.recognize(x, m), args.iters, 2)
            plain = SpeechToTextRecognizer(model, apply_cache=True, max_len=args.plain_max_len, **common)
            t_plain, _ = timed(lambda: plain.recognize(x, m), max(2, args.iters // 2), 1)
            t_enc, _ = timed(lambda: plain.encode(x, m), args.iters, 1)
        n_rows = packed[2].float()
        res[str(B)] = {
            'encoder_ctc_head_ms': t_head, 'search_ms': t_search, 'pack_ms': t_pack, 'decoder_output_ms': t_dec, 'lm_ms': t_lm,
            'score_select_ms': t_sel, 'second_pass_ms': t_pack + t_dec + t_lm + t_sel, 'search_plus_second_pass_ms': t_pass,
            'two_pass_s_per_batch': t_two, 'two_pass_utt_per_s': B / t_two,
            'cached_beam_s_per_batch': t_plain, 'cached_beam_utt_per_s': B / t_plain,
            'cached_beam_ms_per_step': (t_plain - t_enc) * 1e3 / args.plain_max_len,
            'speedup': t_plain / t_two, 'rescorable_fraction': float((n_rows > 0).float().mean()),
            'mean_rows_per_hypothesis': float(n_rows[n_rows > 0].mean()) if bool((n_rows > 0).any()) else 0.0,
            'decoder_rows': int(B * W * args.max_len), 'T_prime': int(lp.shape[1])}
    out = {'metric': 'two-pass decode (CTC n-best W %d K %d + attention / LM rescoring, max_len %d) beside the cached beam search '
                     '(beam %d, max_len %d), C5 shape' % (W, args.cutoff, args.max_len, W, args.plain_max_len),
           'value': res[str(max(int(b) for b in res))]['two_pass_utt_per_s'], 'unit': 'utt/s', 'dtype': args.mode, 'batches': res,
           'iters': args.iters}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out) + '\n')
    return out


if __name__ == '__main__':
    main()
