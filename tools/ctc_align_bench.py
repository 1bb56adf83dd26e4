"""CTC forced alignment benchmark (ops.ctc_forced_align, otr_ctc_align): batch 32 x T' 250 x V 4233 with about 20 labels per
utterance, and the same batch at T' = 349 (the longest AISHELL shape README.md quotes), on peaky random log-probs.  In the same run it
times otr_ctc_loss forward-only (dlogits = NULL) on the same tensors: the same recurrence length on code that exists already, the
yardstick the alignment is read against.  Warm-up, then timed repeats with device events around each launch; medians.  Prints one
JSON line per shape.

    python tools/ctc_align_bench.py [--batch 32] [--frames 250 349] [--vocab 4233] [--labels 20] [--iters 50] [--out f.json]
    python tools/ctc_align_bench.py --profile-once     # one alignment and one loss forward per shape (run under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L, ops      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, nargs='+', default=[250, 349])
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--labels', type=int, default=20, help='labels per utterance: uniform in [labels - 4, labels + 4]')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--profile-once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_align_bench needs a GPU')
    dev = 'cuda'
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)        # noqa: E731
    med = lambda x: float(np.median(x))                                         # noqa: E731
    lines = []
    for T in a.frames:
        B, V = a.batch, a.vocab
        rng = np.random.default_rng(0)
        lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32) * 4.0), -1).to(dev)
        n = rng.integers(max(a.labels - 4, 1), a.labels + 5, size=B)
        max_tgt = int(n.max())
        tg = torch.from_numpy(rng.integers(1, V, size=(B, max_tgt))).to(dev)
        tl = torch.from_numpy(n.astype(np.int32)).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        ws_bytes = lib.otr_ctc_align_workspace_bytes(B, T, max_tgt)
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        ft = torch.empty((B, T), dtype=torch.int32, device=dev)
        sp = torch.empty((B, max_tgt, 2), dtype=torch.int32, device=dev)
        ll = torch.empty((B, max_tgt), dtype=torch.float32, device=dev)
        sc = torch.empty((B,), dtype=torch.float32, device=dev)
        alpha = torch.empty((B, T, 2 * max_tgt + 1), dtype=torch.float32, device=dev)
        nll = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)

        def align():
            L.check(lib.otr_ctc_align(p(lp), V, p(tg), max_tgt, p(il), p(tl), B, T, V, max_tgt, 0, p(ws), ws_bytes, p(ft), p(sp), p(ll),
                                      p(sc), stream()), 'otr_ctc_align')

        def loss_fwd():
            L.check(lib.otr_ctc_loss(p(lp), p(tg), max_tgt, p(il), p(tl), B, T, V, max_tgt, 0, p(alpha), p(nll), p(loss), None, stream()),
                    'otr_ctc_loss')

        if a.profile_once:
            align()
            loss_fwd()
            torch.cuda.synchronize()
            lines.append(json.dumps({'profile_once': True, 'batch': B, 'frames': T, 'vocab': V, 'max_tgt': max_tgt}))
            continue
        for _ in range(a.warmup):
            align()
            loss_fwd()
            ops.ctc_forced_align(lp, il, tg, tl)
        torch.cuda.synchronize()
        t_align, t_loss, t_op = [], [], []
        for _ in range(a.iters):                       # alternate the two, so both see the same clocks and cache state
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            align()
            e[1].record()
            loss_fwd()
            e[2].record()
            torch.cuda.synchronize()
            t_align.append(e[0].elapsed_time(e[1]))
            t_loss.append(e[1].elapsed_time(e[2]))
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.ctc_forced_align(lp, il, tg, tl)
            e1.record()
            torch.cuda.synchronize()
            t_op.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(sc).all()) and bool((sc <= -nll + 1e-5 * nll.abs() + 1e-3).all())       # the best path never beats the sum of all paths
        lines.append(json.dumps({
            'batch': B, 'frames': T, 'vocab': V, 'max_tgt': max_tgt, 'mean_labels': round(float(n.mean()), 1), 'iters': a.iters,
            'align_ms_median': round(med(t_align), 4), 'align_ms_min': round(min(t_align), 4),
            'ctc_loss_fwd_ms_median': round(med(t_loss), 4), 'ctc_loss_fwd_ms_min': round(min(t_loss), 4),
            'align_over_loss_fwd': round(med(t_align) / med(t_loss), 3),
            'op_ms_median': round(med(t_op), 4), 'align_us_per_frame': round(med(t_align) * 1e3 / T, 3),
            'device': torch.cuda.get_device_name(0)}))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
