"""Edit-distance scoring benchmark (ops.edit_distance, otr_edit_distance): 32 utterances x 10 hypotheses of about 20 tokens (the C5
decode shape), 32 x 10 of about 250 tokens, and one 2048 x 2048 pair.  Beside each, in the same run, the host route it replaces for
the same pairs: .cpu() of the token tensors plus the pure-Python Levenshtein table (tests/edit_distance_ref.py; the numpy row form for
the 2048-long pair, where pure Python takes seconds).  It imports that restatement, so it runs from a checkout with tests/ beside
tools/.  Warm-up, then timed repeats with device events; medians.  Two device figures: `call` brackets ops.edit_distance (its two
output allocations and the Python around the launch included: at the small shape mostly that), `launch` brackets the bare
otr_edit_distance call on preallocated outputs.  Neither is a kernel time: that comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/edit_distance_bench.py --profile-once`.  The device's distances are checked against
the host's.  Prints one JSON line per shape.

    python tools/edit_distance_bench.py [--iters 50] [--host-iters 3] [--out f.json] [--profile-once]
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
from opentransformer_amd import _lib as L, ops          # noqa: E402
from tests import edit_distance_ref as ref_impl         # noqa: E402

SHAPES = [('c5_decode', 32, 10, 20, 4, 4233), ('long', 32, 10, 250, 30, 4233), ('limit', 1, 1, 2048, 0, 4)]


def make(rng, B, N, mean, spread, V):
    """references of mean +- spread tokens; hypotheses = the reference with about 15 % of substitutions, deletions and insertions"""
    rl = rng.integers(mean - spread, mean + spread + 1, size=B)
    Lr = int(rl.max())
    ref = rng.integers(2, V, size=(B, Lr))
    hyps, hl = [], np.zeros((B, N), np.int64)
    for b in range(B):
        row = []
        for n in range(N):
            h = []
            for t in ref[b, :rl[b]]:
                u = rng.random()
                if u < 0.05:
                    continue
                h.append(int(rng.integers(2, V)) if u < 0.10 else int(t))
                if u > 0.95:
                    h.append(int(rng.integers(2, V)))
            h = h[:ops.EDIT_MAX_LEN]
            hl[b, n] = len(h)
            row.append(h)
        hyps.append(row)
    Lh = max(int(hl.max()), 1)
    hyp = np.zeros((B, N, Lh), np.int64)
    for b in range(B):
        for n in range(N):
            hyp[b, n, :hl[b, n]] = hyps[b][n]
    return ref, rl.astype(np.int32), hyp, hl.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--profile-once', action='store_true', help='one launch per shape and nothing else: for a kernel trace')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('edit_distance_bench needs a GPU')
    dev = 'cuda'
    med = lambda x: float(np.median(x))                 # noqa: E731
    lines = []
    for name, B, N, mean, spread, V in SHAPES:
        rng = np.random.default_rng(0)
        ref, rl, hyp, hl = make(rng, B, N, mean, spread, V)
        d_ref, d_rl, d_hyp, d_hl = (torch.from_numpy(x).to(dev) for x in (ref, rl, hyp, hl))
        totals = torch.zeros(8, dtype=torch.int64, device=dev)
        o_dist = torch.empty((B, N), dtype=torch.int32, device=dev)
        o_counts = torch.empty((B, N, 3), dtype=torch.int32, device=dev)
        lib = L.load()
        p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

        def launch():
            L.check(lib.otr_edit_distance(p(d_ref), d_ref.stride(0), p(d_rl), p(d_hyp), d_hyp.stride(0), d_hyp.stride(1), p(d_hl), B, N,
                                          d_ref.shape[1], d_hyp.shape[2], -1, p(o_dist), p(o_counts), p(totals),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_edit_distance')

        if a.profile_once:
            launch()
            torch.cuda.synchronize()
            lines.append(json.dumps({'profile_once': True, 'shape': name, 'utterances': B, 'nbest': N}))
            continue
        for _ in range(a.warmup):
            ops.edit_distance(d_ref, d_rl, d_hyp, d_hl, totals=totals)
            launch()
        torch.cuda.synchronize()
        t_launch = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            t_launch.append(e0.elapsed_time(e1))
        t_dev = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dist, counts, _ = ops.edit_distance(d_ref, d_rl, d_hyp, d_hl, totals=totals)
            e1.record()
            torch.cuda.synchronize()
            t_dev.append(e0.elapsed_time(e1))
        fn = ref_impl.pair_fast if name == 'limit' else ref_impl.pair
        t_host, want = [], None
        for _ in range(a.host_iters):                   # the route the kernel replaces: tokens to the host, then the table in Python
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_ref, h_rl, h_hyp, h_hl = d_ref.cpu(), d_rl.cpu(), d_hyp.cpu(), d_hl.cpu()
            want = ref_impl.batch(h_ref.numpy(), h_rl.numpy(), h_hyp.numpy(), h_hl.numpy(), fn=fn)
            t_host.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(dist.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1]), name
        cells = float(sum(int(rl[b]) * int(hl[b, n]) for b in range(B) for n in range(N)))
        rows = float(sum(int(rl[b]) for b in range(B)) * N)
        lines.append(json.dumps({
            'shape': name, 'utterances': B, 'nbest': N, 'mean_ref_tokens': round(float(rl.mean()), 1),
            'mean_hyp_tokens': round(float(hl.mean()), 1), 'iters': a.iters,
            'call_ms_median': round(med(t_dev), 4), 'call_ms_min': round(min(t_dev), 4),
            'launch_ms_median': round(med(t_launch), 4), 'launch_ms_min': round(min(t_launch), 4),
            'host_route': 'cpu() + ' + ('numpy rows' if name == 'limit' else 'pure Python'), 'host_ms_median': round(med(t_host), 3),
            'host_over_call': round(med(t_host) / med(t_dev), 1),
            'table_rows_per_s': round(rows / (med(t_launch) * 1e-3), 0), 'cells_per_s': round(cells / (med(t_launch) * 1e-3), 0),
            'device': torch.cuda.get_device_name(0)}))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
