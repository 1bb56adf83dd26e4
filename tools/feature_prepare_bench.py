"""Feature-preparation benchmark (otr_feature_prepare, data.FeaturePipeline): utterance normalisation + SpecAugment + padding of a batch
of raw features, at 32 x 1000 x 80 (the bench batch), a ragged batch of 32 with 600 .. 1400 frames, and F = 40.  Three figures per
shape, one JSON line:
 * `entry`: the bare otr_feature_prepare call (mode 1, the recipe's rectangles) on a device-resident packed buffer and preallocated
   outputs, with its bytes -- two reads of the live values and one write of the padded batch -- and the read-once / write-once minimum
   over time against the achievable HBM rate (6.3 TB/s);
 * `pipeline`: data.FeaturePipeline from the utterances, host draws, uploads and target assembly included;
 * `composed`: the path available without it -- data.collate_fn_with_eos_bos, then torch.std_mean normalisation of every utterance on
   the device, then data.spec_augment_batch.
`pipeline` and `composed` are timed from host-resident utterances (what a DataLoader hands over) and from device-resident ones.  All
paths run in the same process, alternating in rounds after a warm-up, with device events around each round; medians of the per-call
time over the rounds.  The two paths' outputs are compared under the same seeds before timing.

    python tools/feature_prepare_bench.py [--rounds 10] [--calls 20] [--out profiles/feature_prepare_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import _lib as L, data           # noqa: E402

HBM_BYTES_PER_S = 6.3e12      # achievable rate of the MI355X's HBM
SPEC = dict(freq_mask_num=2, time_mask_num=5, freq_mask_rate=0.3, time_mask_rate=0.05)    # transformer_baseline.yaml
PARAMS = dict(normalization=True, gaussian_noise=0.0, spec_augment=True, spec_augment_config=SPEC)
DEV = 'cuda'


def make_batch(lengths, F_, seed):
    rng = np.random.default_rng(seed)
    return [('utt%d' % i, torch.from_numpy((rng.standard_normal((T, F_)) * 3 + 5).astype(np.float32)), T,
             [int(v) for v in rng.integers(3, 4000, 15)], 15) for i, T in enumerate(lengths)]


def composed(batch):
    utt_ids, inputs, targets = data.collate_fn_with_eos_bos(batch, DEV)
    feats = inputs['inputs']
    for b, d in enumerate(batch):
        x = feats[b, :d[2]]
        std, mean = torch.std_mean(x)
        x.sub_(mean).div_(std)
    data.spec_augment_batch(feats, [d[2] for d in batch], **SPEC)
    return utt_ids, inputs, targets


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def rounds(fns, n_rounds, calls):
    """{name: median ms per call}: the paths alternate round by round, device events around each round of `calls` calls"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / calls)
    return {k: float(np.median(v)) for k, v in ts.items()}


def entry_call(batch, Tmax, F_):
    lib = L.load()
    B = len(batch)
    lengths = [d[2] for d in batch]
    src = torch.cat([d[1] for d in batch]).to(DEV)
    off = torch.tensor(np.concatenate(([0], np.cumsum(lengths[:-1]))), dtype=torch.int64, device=DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    seed_all(0)
    ranges = torch.tensor([data.spec_augment_ranges(T, F_, **SPEC) for T in lengths], dtype=torch.int32, device=DEV)
    dst = torch.empty((B, Tmax, F_), dtype=torch.float32, device=DEV)
    mask = torch.empty((B, Tmax), dtype=torch.uint8, device=DEV)
    nws = lib.otr_feature_prepare_workspace_bytes(B, Tmax, F_)
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731

    def call():
        L.check(lib.otr_feature_prepare(p(src), p(off), p(ln), B, Tmax, F_, 1, None, None, None, p(ranges), ranges.shape[1], p(dst), p(mask),
                                        None, p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_feature_prepare')
    live = sum(lengths) * F_ * 4
    return call, {'bytes_moved': 2 * live + B * Tmax * F_ * 4, 'bytes_minimum': live + B * Tmax * F_ * 4}


def bench_shape(name, lengths, F_, a):
    batch = make_batch(lengths, F_, len(name))
    on_dev = [(u, f.to(DEV), T, t, tl) for u, f, T, t, tl in batch]
    pipe = data.FeaturePipeline(PARAMS)
    # same seeds, same batch: the two paths agree (zero pattern exactly, values to float32 rounding)
    seed_all(1)
    _, got, _ = pipe(batch, DEV)
    seed_all(1)
    _, want, _ = composed(batch)
    x, y = got['inputs'], want['inputs']
    assert torch.equal(x == 0, y == 0) and torch.equal(got['mask'], want['mask'])
    assert float((x - y).abs().max()) < 1e-4, float((x - y).abs().max())
    call, traffic = entry_call(batch, max(lengths), F_)
    t = rounds({'entry': call, 'pipeline_host': lambda: pipe(batch, DEV), 'composed_host': lambda: composed(batch),
                'pipeline_device': lambda: pipe(on_dev, DEV), 'composed_device': lambda: composed(on_dev)}, a.rounds, a.calls)
    res = {'B': len(lengths), 'Tmax': max(lengths), 'F': F_, 'frames': int(sum(lengths))}
    res.update({k + '_ms': round(v, 4) for k, v in t.items()})
    res.update(traffic)
    res['entry_moved_TBps'] = round(traffic['bytes_moved'] / (t['entry'] * 1e-3) / 1e12, 3)
    res['entry_minimum_TBps'] = round(traffic['bytes_minimum'] / (t['entry'] * 1e-3) / 1e12, 3)
    res['entry_minimum_over_hbm_rate'] = round(traffic['bytes_minimum'] / (t['entry'] * 1e-3) / HBM_BYTES_PER_S, 3)
    res['composed_over_pipeline_host'] = round(t['composed_host'] / t['pipeline_host'], 2)
    res['composed_over_pipeline_device'] = round(t['composed_device'] / t['pipeline_device'], 2)
    res['pipeline_not_slower_than_composed'] = bool(t['pipeline_host'] <= t['composed_host'] and t['pipeline_device'] <= t['composed_device'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--calls', type=int, default=20, help='calls per round; rounds * calls >= 200 calls per path')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feature_prepare_bench needs a GPU')
    rng = np.random.default_rng(0)
    ragged = [int(v) for v in rng.integers(600, 1401, 32)]
    res = {'calls_per_path': a.rounds * a.calls, 'hbm_rate_TBps': HBM_BYTES_PER_S / 1e12,
           'bench_32x1000x80': bench_shape('bench', [1000] * 32, 80, a),
           'ragged_32x600-1400x80': bench_shape('ragged', ragged, 80, a),
           'f40_32x1000x40': bench_shape('f40', [1000] * 32, 40, a),
           'device': torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
