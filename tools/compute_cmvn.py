"""Global CMVN statistics of a feature corpus on the device (data.GlobalCMVN, otr_cmvn_accumulate): writes `<prefix>.mean.npy` and
`<prefix>.std.npy`, the two files the `global_cmvn: <prefix>` key of a recipe's data section names (otrans/data/audio.py:43-45 loads
them; data.FeaturePipeline does the same).  Population std, Kaldi's convention.

    python tools/compute_cmvn.py --out exp/cmvn feats/utt1.npy feats/utt2.npy ...      # one [T, F] float matrix per file
    python tools/compute_cmvn.py --out exp/cmvn feats.npz                               # or one archive of such matrices

Utterances are uploaded `--batch-size` at a time as one packed buffer; the sums stay on the device in float64 until the end.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import data                    # noqa: E402


def matrices(paths):
    if len(paths) == 1 and paths[0].endswith('.npz'):
        with np.load(paths[0], allow_pickle=False) as z:
            for k in z.files:
                yield z[k]
    else:
        for p in paths:
            yield np.load(p, allow_pickle=False)


def compute(paths, batch_size, device):
    """data.GlobalCMVN over the matrices of `paths`"""
    cm, group = None, []

    def flush():
        lengths = [m.shape[0] for m in group]
        src = torch.from_numpy(np.concatenate(group).astype(np.float32, copy=False)).to(device)
        off = torch.tensor(np.concatenate(([0], np.cumsum(lengths[:-1]))), dtype=torch.int64, device=device)
        cm.update(src, off, torch.tensor(lengths, dtype=torch.int32, device=device))
        group.clear()
    for m in matrices(paths):
        if m.ndim != 2 or (cm is not None and m.shape[1] != cm.F):
            raise SystemExit('compute_cmvn: every input must be a [T, F] matrix with the same F, got %s' % (m.shape,))
        if cm is None:
            cm = data.GlobalCMVN(m.shape[1], device)
        group.append(m)
        if len(group) == batch_size:
            flush()
    if cm is None:
        raise SystemExit('compute_cmvn: no input')
    if group:
        flush()
    return cm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('inputs', nargs='+', help='.npy feature matrices [T, F], or one .npz of them')
    ap.add_argument('--out', required=True, help='output prefix: writes <out>.mean.npy and <out>.std.npy')
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args()
    cm = compute(a.inputs, max(a.batch_size, 1), a.device)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cm.save(a.out)
    print('compute_cmvn: %d frames, F = %d -> %s.mean.npy, %s.std.npy' % (int(cm.acc[2 * cm.F]), cm.F, a.out, a.out))


if __name__ == '__main__':
    main()
