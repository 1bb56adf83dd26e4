"""N-best consensus benchmark (ops.nbest_consensus, otr_nbest_consensus: token confidences and MBR risks): 32 utterances x 10
hypotheses of about 20 tokens (the C5 decode shape's n-best), 32 x 10 of about 252 tokens, and 32 x 32 of about 20 tokens.  Per
shape, in one run, three figures for the device -- `call` brackets ops.nbest_consensus (its four output allocations and the Python
around its two launches included) between two device events, `graph` is the two launches as nodes of one captured graph, 50 of
them per replay, per call -- and two yardsticks:
  * the host restatement: .cpu() of the token tensors plus the pure-Python loop of tests/nbest_consensus_ref.py over the same pairs;
  * ops.edit_distance on the same B * N * N pairs (hypothesis i against hypothesis j as the reference), also as graph nodes: that
    kernel takes the distance only, so its time is the floor for the row sweep and the ratio to it is what the back-pointers, the
    walk back and the sums cost.
The device's outputs are checked against the restatement, and its risks against sum_j post[j] * (edit_distance's dist), before
anything is reported.
--decode adds the cost of mbr=True in a decode: recognize_tokens() of the cached search at the C5 decode shape of tools/bias_bench.py
(batch 32, beam 10, T' 249, max_len 60, fp16) with mbr=False and mbr=True in alternating blocks, and the MBR tail alone (the consensus,
the sort and the gathers on the final beam).  --parent-lib times the decode STEP of the mbr=False recognizer against the parent
commit's library in the same blocks, both builds twice, as tools/bias_bench.py does: the default path launches what it launched.
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/consensus_bench.py --profile-once`.

    python tools/consensus_bench.py [--iters 50] [--host-iters 1] [--decode] [--parent-lib DIR_OR_SO] [--out f.json] [--profile-once]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L, ops                     # noqa: E402
from tests import nbest_consensus_ref as ref_impl                  # noqa: E402
from tools.edit_distance_bench import make                         # noqa: E402
from tools.ngram_attn_bench import V, Step, build, event_ms, foreign_lib, kernel_us      # noqa: E402

SHAPES = [('c5_decode', 32, 10, 20, 4), ('long', 32, 10, 250, 6), ('wide', 32, 32, 20, 4)]


def nbest(rng, B, N, mean, spread):
    """an n-best per utterance: the hypotheses tools/edit_distance_bench.py makes (a base string with about 15 % of errors), cut to
    the limit, and descending normal scores"""
    _, _, hyp, hl = make(rng, B, N, mean, spread, 4233)
    hyp, hl = hyp[:, :, :ops.NBEST_MAX_LEN], np.minimum(hl, ops.NBEST_MAX_LEN)
    scores = -np.sort(-(rng.standard_normal((B, N)) * 2.0).astype(np.float32), axis=1)
    return hyp, hl.astype(np.int32), scores


def shapes(a, dev):
    med = lambda x: float(np.median(x))                             # noqa: E731
    out = []
    for name, B, N, mean, spread in SHAPES:
        tokens, lengths, scores = nbest(np.random.default_rng(0), B, N, mean, spread)
        d_tok, d_len, d_sc = (torch.from_numpy(x).to(dev) for x in (tokens, lengths, scores))
        if a.profile_once:
            ops.nbest_consensus(d_tok, d_len, d_sc)
            torch.cuda.synchronize()
            out.append({'profile_once': True, 'shape': name, 'utterances': B, 'nbest': N})
            continue
        for _ in range(a.warmup):
            got = ops.nbest_consensus(d_tok, d_len, d_sc)
        torch.cuda.synchronize()
        t_call = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = ops.nbest_consensus(d_tok, d_len, d_sc)
            e1.record()
            torch.cuda.synchronize()
            t_call.append(e0.elapsed_time(e1))
        graph_us = kernel_us(lambda: ops.nbest_consensus(d_tok, d_len, d_sc))
        # the same pairs through the distance-only kernel: reference (b, j), its hypotheses all N of utterance b
        L_ = d_tok.shape[2]
        e_ref, e_len = d_tok.reshape(B * N, L_), d_len.reshape(B * N)
        e_hyp, e_hl = d_tok[:, None].expand(B, N, N, L_).reshape(B * N, N, L_), d_len[:, None].expand(B, N, N).reshape(B * N, N)
        totals = torch.zeros(8, dtype=torch.int64, device=dev)
        dist_us = kernel_us(lambda: ops.edit_distance(e_ref, e_len, e_hyp, e_hl, totals=totals))
        dist = ops.edit_distance(e_ref, e_len, e_hyp, e_hl)[0].reshape(B, N, N).double()         # [b, j, i]
        risk_check = (got[0].double().unsqueeze(-1) * dist).sum(1)
        assert torch.allclose(risk_check, got[1].double(), rtol=0, atol=1e-6 * (1 + L_)), name
        t_host, want = [], None
        for _ in range(a.host_iters):                               # the route the kernel replaces: tokens to the host, then Python
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = ref_impl.consensus(d_tok.cpu().numpy(), d_len.cpu().numpy(), d_sc.cpu().numpy())
            t_host.append((time.perf_counter() - t0) * 1e3)
        post, risk, best, conf = (t.cpu().numpy() for t in got)
        assert np.array_equal(best, want[2]) and np.abs(post - want[0]).max() <= 1e-6 and np.abs(conf - want[3]).max() <= 4e-6, name
        assert np.abs(risk - want[1]).max() <= 1e-6 * (1 + L_), name
        cells = float(sum(int(lengths[b, i]) * int(lengths[b, j]) for b in range(B) for i in range(N) for j in range(N) if i != j))
        out.append({'shape': name, 'utterances': B, 'nbest': N, 'pairs': B * N * N, 'mean_tokens': round(float(lengths.mean()), 1),
                    'iters': a.iters, 'call_ms_median': round(med(t_call), 4), 'call_ms_min': round(min(t_call), 4),
                    'graph_us_per_call': round(graph_us, 2), 'edit_distance_graph_us_per_call': round(dist_us, 2),
                    'consensus_over_edit_distance': round(graph_us / dist_us, 3),
                    'host_route': 'cpu() + pure Python / numpy rows', 'host_ms_median': round(med(t_host), 1),
                    'host_over_call': round(med(t_host) / med(t_call), 1), 'cells_per_s': round(cells / (graph_us * 1e-6), 0)})
    return out


def decode(a, dev):
    """mbr=True against mbr=False in the cached decode of the C5 shape, and the default path's step against the parent build"""
    from opentransformer_amd import recognize
    from opentransformer_amd import synthetic as syn
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    model, lm = build('fp16', dev)
    inputs, _ = syn.synthetic_batch(a.batch, 1000, 80, V, 15, seed=0)
    x, m = inputs['inputs'].to(dev), inputs['mask'].to(dev)
    kw = dict(beam_width=10, nbest=1, max_len=60, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, ctc_weight=0.3,
              idx2unit={i: str(i) for i in range(V)}, apply_cache=True)
    recs = {'mbr_off': SpeechToTextRecognizer(model, **kw), 'mbr_on': SpeechToTextRecognizer(model, mbr=True, **kw)}
    with torch.no_grad():
        for r in recs.values():                                     # eager visits, then the captures
            for _ in range(3):
                r.recognize_tokens(x, m)
        torch.cuda.synchronize()
        blocks = {k: [] for k in recs}
        for _ in range(a.blocks):
            for k, r in recs.items():
                blocks[k].append(event_ms(lambda: r.recognize_tokens(x, m), 5))
        beam = recs['mbr_off']._beam_device(x, m, 10)
        tail = event_ms(lambda: recognize._consensus_nbest(*beam, 1.0, True, 1, recognize.EOS), a.iters)
        tail_graph = kernel_us(lambda: recognize._consensus_nbest(*beam, 1.0, True, 1, recognize.EOS))
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    res = {'decode_shape': 'C5 with a CTC head, batch %d, beam 10, TransformerLM, max_len 60, fp16, cached search' % a.batch,
           'final_beam_token_width': int(beam[0].shape[2]), 'recognize_tokens_ms_blocks': {k: [round(t, 3) for t in v] for k, v in blocks.items()},
           'recognize_tokens_ms_median': {k: round(v, 3) for k, v in med.items()},
           'mbr_on_minus_off_ms': round(med['mbr_on'] - med['mbr_off'], 3), 'mbr_tail_alone_ms': round(tail, 4),
           'mbr_tail_alone_graph_us': round(tail_graph, 2)}
    if a.parent_lib:
        kw1 = dict(kw)
        steps = {'plain': Step(SpeechToTextRecognizer(model, **kw1), x, m), 'joint': Step(SpeechToTextRecognizer(model, joint_ctc=True, **kw1), x, m)}
        ours = L.load('fp16')
        for again in ('', '_again'):
            L._libs['fp16'] = foreign_lib(a.parent_lib, 'fp16')     # the parent's kernels go into the graphs captured now
            try:
                for tag, joint in (('parent_plain', False), ('parent_joint', True)):
                    steps[tag + again] = Step(SpeechToTextRecognizer(model, joint_ctc=joint, **kw1), x, m)
            finally:
                L._libs['fp16'] = ours
            if not again:
                for tag, joint in (('plain_again', False), ('joint_again', True)):
                    steps[tag] = Step(SpeechToTextRecognizer(model, joint_ctc=joint, **kw1), x, m)
        ms = {k: [] for k in steps}
        for _ in range(a.blocks):
            for k, s in steps.items():
                ms[k].append(s.block(a.iters))
        best = lambda k: float(np.median(ms[k]))                    # noqa: E731
        res.update(step_ms_median={k: round(best(k), 4) for k in steps}, step_ms_blocks={k: [round(v, 4) for v in ms[k]] for k in steps},
                   plain_over_parent=round(best('plain') / best('parent_plain'), 4),
                   plain_again_over_parent=round(best('plain_again') / best('parent_plain'), 4),
                   parent_plain_again_over_parent=round(best('parent_plain_again') / best('parent_plain'), 4),
                   joint_over_parent=round(best('joint') / best('parent_joint'), 4),
                   joint_again_over_parent=round(best('joint_again') / best('parent_joint'), 4),
                   parent_joint_again_over_parent=round(best('parent_joint_again') / best('parent_joint'), 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--decode', action='store_true', help='also the cost of mbr=True in the cached decode of the C5 shape')
    ap.add_argument('--parent-lib', default=None, help='with --decode: the parent commit\'s library (a .so of the fp16 build, or the '
                                                       'directory holding both builds); its decode steps are timed in the same blocks, twice')
    ap.add_argument('--profile-once', action='store_true', help='one call per shape and nothing else: for a kernel trace')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('consensus_bench needs a GPU')
    dev = torch.device('cuda:0')
    lines = [json.dumps(dict(r, device=torch.cuda.get_device_name(0))) for r in shapes(a, dev)]
    if a.decode and not a.profile_once:
        lines.append(json.dumps(dict(decode(a, dev), device=torch.cuda.get_device_name(0))))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
