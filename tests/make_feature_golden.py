#!/usr/bin/env python3
"""Write tests/golden/feature_chain.npz: the reference's per-utterance feature chain (otrans/data/audio.py:125-136) on three small
utterances.  TEST INFRASTRUCTURE, run once where the reference checkout is available (never on the GPU machine):

    python tests/make_feature_golden.py /path/to/reference

otrans/data/audio.py itself cannot be imported without torchaudio, so its `normalization` (audio.py:22-24), its global-CMVN line
(audio.py:127) and its noise draw (audio.py:132-133) are restated here line for line; `spec_augment` is the reference's own function.
The order per utterance is the reference's: normalise, draw and add the noise, then SpecAugment; the generators are seeded once
before the first utterance, as in a seeded single-process run."""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('OTRANS_REFERENCE', '')
assert os.path.isdir(os.path.join(REFERENCE, 'otrans')), 'usage: make_feature_golden.py <reference checkout>'
sys.path.insert(0, REFERENCE)

from otrans.data.augment import spec_augment            # noqa: E402

SEED, SIGMA, F = 20, 0.25, 8
LENGTHS = [40, 23, 31]


def normalization(feature):                             # audio.py:22-24
    std, mean = torch.std_mean(feature)
    return (feature - mean) / std


def seed_all():
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    random.seed(SEED)


def run_chain(feats, normalise):
    seed_all()
    out, noises = [], []
    for x in feats:
        feature = normalise(x.clone())
        noise = torch.normal(torch.zeros(feature.size(-1)), std=SIGMA)       # audio.py:132-133
        feature += noise
        feature = spec_augment(feature)                                      # audio.py:136 (its default configuration)
        out.append(feature.numpy())
        noises.append(noise.numpy())
    return out, noises


def main():
    rng = np.random.default_rng(SEED)
    feats = [torch.from_numpy((rng.standard_normal((T, F)) * (1.5 + b) + 3.0 * (b - 1) + np.arange(F)).astype(np.float32))
             for b, T in enumerate(LENGTHS)]
    allx = np.concatenate([x.numpy().astype(np.float64) for x in feats])
    gmean = torch.from_numpy(allx.mean(0).astype(np.float32))
    gstd = torch.from_numpy(allx.std(0).astype(np.float32))                  # population std (Kaldi); the reference defines none
    out = {'seed': np.int64(SEED), 'sigma': np.float64(SIGMA), 'lengths': np.asarray(LENGTHS, np.int64),
           'gmean': gmean.numpy(), 'gstd': gstd.numpy()}
    utt, noises = run_chain(feats, normalization)
    glob, noises_g = run_chain(feats, lambda x: (x - gmean) / gstd)          # audio.py:127
    for b, x in enumerate(feats):
        assert np.array_equal(noises[b], noises_g[b])
        out['x%d' % b] = x.numpy()
        out['norm_utt%d' % b] = normalization(x).numpy()
        out['norm_glob%d' % b] = ((x - gmean) / gstd).numpy()
        out['noise%d' % b] = noises[b]
        out['chain_utt%d' % b] = utt[b]
        out['chain_glob%d' % b] = glob[b]
    zeros = sum(int((a == 0).sum()) for a in utt)
    assert zeros > 0, 'the seed draws no mask of non-zero size'
    path = os.path.join(HERE, 'golden', 'feature_chain.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', zeros, 'masked cells')


if __name__ == '__main__':
    main()
