"""CTC prefix beam search benchmark (CTCRecognizer mode='beam'): batch 32 x T' 250 x V 4233, beam 10, cutoff_top_n 40, on peaky
random log-probs.  Times the two launches with device events around each (the top-K pass over [B*T', V], the one-launch search)
and the pair as ops.ctc_prefix_beam_search is called, reports the bytes the top-K pass must read, and times the plain-Python
restatement (tests/ctc_prefix_ref.py) on the same batch; the 1-best of every utterance is compared.  Prints one JSON line.

    python tools/ctc_beam_bench.py [--batch 32] [--frames 250] [--vocab 4233] [--beam 10] [--topk 40] [--iters 50] [--out f.json]
    python tools/ctc_beam_bench.py --profile-once     # one decode batch, nothing else (run under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L, ops      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--topk', type=int, default=40)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cpu-utts', type=int, default=None, help='utterances the CPU restatement decodes (default: all)')
    ap.add_argument('--profile-once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_beam_bench needs a GPU')
    dev = 'cuda'
    B, T, V, W, K = a.batch, a.frames, a.vocab, a.beam, a.topk
    rng = np.random.default_rng(0)
    lp_host = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * 4.0), -1)
    lp = lp_host.to(dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    if a.profile_once:
        ops.ctc_prefix_beam_search(lp, ln, beam_width=W, cutoff_top_n=K)
        torch.cuda.synchronize()
        print(json.dumps({'profile_once': True, 'batch': B, 'frames': T, 'vocab': V, 'beam': W, 'topk': K}))
        return
    lib = L.load()
    top_lp = torch.empty((B * T, K), dtype=torch.float32, device=dev)
    top_tok = torch.empty((B * T, K), dtype=torch.int32, device=dev)
    ws_bytes = lib.otr_ctc_beam_workspace_bytes(B, T, W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    tokens = torch.empty((B, W, T), dtype=torch.int64, device=dev)
    out_len = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

    def topk():
        L.check(lib.otr_ctc_topk(p(lp), V, p(ln), B, T, V, K, p(top_lp), p(top_tok), stream()), 'otr_ctc_topk')

    def search():
        L.check(lib.otr_ctc_beam_search(p(top_lp), p(top_tok), p(ln), B, T, V, K, 0, W, p(ws), ws_bytes, p(tokens), p(out_len),
                                        p(scores), stream()), 'otr_ctc_beam_search')

    for _ in range(a.warmup):
        topk()
        search()
        ops.ctc_prefix_beam_search(lp, ln, beam_width=W, cutoff_top_n=K)
    torch.cuda.synchronize()
    t_topk, t_search, t_op = [], [], []
    for _ in range(a.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        topk()
        e[1].record()
        search()
        e[2].record()
        torch.cuda.synchronize()
        t_topk.append(e[0].elapsed_time(e[1]))
        t_search.append(e[1].elapsed_time(e[2]))
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.ctc_prefix_beam_search(lp, ln, beam_width=W, cutoff_top_n=K)
        e1.record()
        torch.cuda.synchronize()
        t_op.append(e0.elapsed_time(e1))
    gpu_best = [tokens[b, 0, :int(out_len[b, 0])].tolist() for b in range(B)]

    from tests import ctc_prefix_ref as ref
    n_cpu = B if a.cpu_utts is None else min(a.cpu_utts, B)
    t0 = time.perf_counter()
    rt, rl, rs = ref.decode(lp_host[:n_cpu].numpy(), [T] * n_cpu, W, K)
    cpu_s = time.perf_counter() - t0
    agree = sum(gpu_best[b] == rt[b, 0, :rl[b, 0]].tolist() for b in range(n_cpu))
    med = lambda x: float(np.median(x))                    # noqa: E731
    read_bytes = B * T * V * 4
    res = {
        'batch': B, 'frames': T, 'vocab': V, 'beam': W, 'topk': K, 'iters': a.iters,
        'topk_ms_median': round(med(t_topk), 4), 'search_ms_median': round(med(t_search), 4),
        'op_ms_median': round(med(t_op), 4), 'op_ms_min': round(min(t_op), 4),
        'topk_read_bytes': read_bytes, 'topk_read_GBps': round(read_bytes / (med(t_topk) * 1e-3) / 1e9, 1),
        'search_us_per_frame': round(med(t_search) * 1e3 / T, 3),
        'cpu_restatement_s': round(cpu_s, 3), 'cpu_restatement_utts': n_cpu,
        'cpu_restatement_ms_per_batch': round(cpu_s * 1e3 * B / n_cpu, 1),
        'one_best_agree': '%d/%d' % (agree, n_cpu),
        'device': torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
