"""CTC segmentation benchmark (ops.ctc_segment, otr_ctc_segment) on peaky random log-probs.
  long:  one recording of 16384 frames x V 4233 with 2048 labels, free ends, and 8 such recordings in one call; skip_logp = -30 makes the
         path cover every frame (the longest back-trace; covered_frames says what it covered).  Beside the call's time:
         the numpy restatement (tests/ctc_segment_ref.py) on the first recording in the same run -- the device outputs must equal it --
         and the forward sweep alone: the same call on log-probs whose first label is -inf everywhere runs every frame of the sweep and
         then finds no finite path, so it has no back-trace and no output passes.  The difference is what the trace and the passes cost.
  short: 32 x 250 frames x ~20 labels with both ends fixed, beside otr_ctc_align on the same tensors (equal outputs asserted).
Warm-up, then timed repeats with device events around each launch, the calls that are compared alternating; medians.  One JSON line
per shape.

    python tools/ctc_segment_bench.py [--frames 16384] [--vocab 4233] [--labels 2048] [--batch 8] [--iters 10] [--out f.json]
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
from tests import ctc_segment_ref as ref             # noqa: E402

NAMES = ('frame_token', 'spans', 'label_logp', 'score', 'bounds')


def timed(calls, iters, warmup):
    """medians and minima [ms] of each of `calls`, run alternately so that all see the same clocks and cache state"""
    for _ in range(warmup):
        for call in calls:
            call()
    torch.cuda.synchronize()
    times = [[] for _ in calls]
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        ev[0].record()
        for k, call in enumerate(calls):
            call()
            ev[k + 1].record()
        torch.cuda.synchronize()
        for k in range(len(calls)):
            times[k].append(ev[k].elapsed_time(ev[k + 1]))
    return [(float(np.median(t)), float(min(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16384)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--labels', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--short', type=int, nargs=3, default=[32, 250, 20], metavar=('B', 'T', 'LABELS'))
    ap.add_argument('--skip-logp', type=float, default=-30.0, help='long case: the default is dearer than any frame of these log-probs, so '
                    'the path covers the whole recording: the longest back-trace')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_segment_bench needs a GPU')
    dev = 'cuda'
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)        # noqa: E731
    r3 = lambda x: round(x, 3)                                                  # noqa: E731
    name = torch.cuda.get_device_name(0)
    lines = []

    # ---------------- long recordings, free ends
    T, V, n = a.frames, a.vocab, a.labels
    gen = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    for B in sorted({1, a.batch}):
        lp = torch.log_softmax(torch.randn((B, T, V), generator=gen, device=dev) * 4.0, -1)
        tg = torch.from_numpy(rng.integers(1, V, size=(B, n))).to(dev)
        tl = torch.full((B,), n, dtype=torch.int32, device=dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        dead = lp.clone()
        dead[torch.arange(B, device=dev), :, tg[:, 0]] = -float('inf')          # every path passes its first label: the sweep runs, nothing is traced
        ws_bytes = lib.otr_ctc_segment_workspace_bytes(B, T, n)
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        out = [torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B, n, 2), dtype=torch.int32, device=dev),
               torch.empty((B, n), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
               torch.empty((B, 2), dtype=torch.int32, device=dev)]

        def segment(x):
            L.check(lib.otr_ctc_segment(p(x), V, p(tg), n, p(il), p(tl), B, T, V, n, 0, 1, 1, a.skip_logp, p(ws), ws_bytes,
                                        *[p(o) for o in out], stream()), 'otr_ctc_segment')

        (t_dead, _), (t_full, t_full_min) = timed([lambda: segment(dead), lambda: segment(lp)], a.iters, a.warmup)
        (t_op, _), = timed([lambda: ops.ctc_segment(lp, il, tg, tl, skip_logp=a.skip_logp)], a.iters, 1)
        segment(lp)
        got = [o[0].cpu().numpy() for o in out]
        assert np.isfinite(got[3])
        line = {'case': 'long', 'batch': B, 'frames': T, 'vocab': V, 'labels': n, 'iters': a.iters,
                'segment_ms_median': r3(t_full), 'segment_ms_min': r3(t_full_min), 'sweep_only_ms_median': r3(t_dead),
                'trace_and_passes_ms': r3(t_full - t_dead), 'op_ms_median': r3(t_op), 'us_per_frame': r3(t_full * 1e3 / T),
                'workspace_mib': r3(ws_bytes / 2 ** 20), 'covered_frames': int(got[4][1] - got[4][0])}
        if B == 1:
            x, labels = lp[0].cpu().numpy(), tg[:1].cpu().numpy()
            t0 = time.perf_counter()
            want = ref.segment(x[None], [T], labels, [n], skip_logp=a.skip_logp)
            line['numpy_restatement_ms'] = r3((time.perf_counter() - t0) * 1e3)
            for nm, g, w in zip(NAMES, got, want):
                np.testing.assert_array_equal(g, w[0], err_msg=nm)
            line['equals_restatement'] = True
            assert t_full < line['numpy_restatement_ms']
        lines.append(json.dumps(dict(line, device=name)))
        del lp, dead, ws

    # ---------------- short utterances, fixed ends, beside otr_ctc_align
    B, T, n = a.short
    lp = torch.log_softmax(torch.randn((B, T, V), generator=gen, device=dev) * 4.0, -1)
    cnt = rng.integers(max(n - 4, 1), n + 5, size=B)
    M = int(cnt.max())
    tg = torch.from_numpy(rng.integers(1, V, size=(B, M))).to(dev)
    tl = torch.from_numpy(cnt.astype(np.int32)).to(dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws_s, ws_a = lib.otr_ctc_segment_workspace_bytes(B, T, M), lib.otr_ctc_align_workspace_bytes(B, T, M)
    ws = torch.empty(max(ws_s, ws_a) // 8 + 1, dtype=torch.int64, device=dev)
    outs = [[torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B, M, 2), dtype=torch.int32, device=dev),
             torch.empty((B, M), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev)] for _ in range(2)]
    bounds = torch.empty((B, 2), dtype=torch.int32, device=dev)

    def seg_fixed():
        L.check(lib.otr_ctc_segment(p(lp), V, p(tg), M, p(il), p(tl), B, T, V, M, 0, 0, 0, 0.0, p(ws), ws_s, *[p(o) for o in outs[0]],
                                    p(bounds), stream()), 'otr_ctc_segment')

    def align():
        L.check(lib.otr_ctc_align(p(lp), V, p(tg), M, p(il), p(tl), B, T, V, M, 0, p(ws), ws_a, *[p(o) for o in outs[1]], stream()),
                'otr_ctc_align')

    (t_seg, t_seg_min), (t_al, t_al_min) = timed([seg_fixed, align], max(a.iters, 50), 5)
    assert all(torch.equal(x, y) for x, y in zip(*outs)) and bool(torch.isfinite(outs[0][3]).all())
    lines.append(json.dumps({'case': 'short_fixed_ends', 'batch': B, 'frames': T, 'vocab': V, 'max_tgt': M,
                             'segment_ms_median': round(t_seg, 4), 'segment_ms_min': round(t_seg_min, 4),
                             'ctc_align_ms_median': round(t_al, 4), 'ctc_align_ms_min': round(t_al_min, 4),
                             'segment_over_align': r3(t_seg / t_al), 'equal_outputs': True, 'device': name}))
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
