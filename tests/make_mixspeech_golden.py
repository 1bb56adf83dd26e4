#!/usr/bin/env python3
"""Write tests/golden/mixspeech_c1.npz: one MixSpeech step of the reference's real SpeechToText (otrans/train/trainer.py:155-201) on the
CPU, for the c1 configuration at dropout 0, once without and once with a CTC head.  TEST INFRASTRUCTURE, run once where the reference
checkout is available (never on the GPU machine):

    python tests/make_mixspeech_golden.py /path/to/reference

The trainer forms the mixed batch inline in its training loop, which cannot be imported: what those lines (trainer.py:156-199) compute
is written out again here, with the reference's draw of lambda from numpy's seeded global generator; the model, its losses and its
backward pass are the reference's own.  Weights are not stored: opentransformer_amd.synthetic.fill_state_dict_ regenerates them."""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('OTRANS_REFERENCE', '')
assert os.path.isdir(os.path.join(REFERENCE, 'otrans')), 'usage: make_mixspeech_golden.py <reference checkout>'
sys.path.insert(0, ROOT)
# the second entry only satisfies the bare `from activation import Swish` at otrans/module/ffn.py:9
sys.path[:0] = [REFERENCE, os.path.join(REFERENCE, 'otrans', 'module')]

from otrans.model import End2EndModel                           # noqa: E402

from opentransformer_amd import synthetic as syn                # noqa: E402

SEED = 31
BATCH = dict(batch=5, frames=96, feat_dim=80, vocab=100, tgt_len=6, seed=7, lengths=[96, 80, 96, 64, 50], tgt_lengths=[6, 4, 5, 6, 3])


def probe_vector(key, numel):
    rng = np.random.default_rng(zlib.crc32(('probe:' + key).encode()))
    return rng.standard_normal(numel).astype(np.float32)


def mixspeech_step(model, inputs, targets):
    """what trainer.py:156-199 does to a batch: the draw (one Beta(0.5, 0.5) value from numpy's global generator, cast to float32), the
    even and odd utterances mixed as even * lam + odd * (1 - lam) in float32, mask and length of the longer, the reference model run on
    the mixed batch once per target set, and the two losses combined with the same weights"""
    n = inputs['inputs'].shape[0] // 2 * 2
    lam = torch.from_numpy(np.random.beta(0.5, 0.5, size=(1))).float()
    even, odd = slice(0, n, 2), slice(1, n, 2)
    x = inputs['inputs']
    mixed = {'inputs': x[even] * lam + x[odd] * (1 - lam),
             'mask': torch.max(inputs['mask'][even], inputs['mask'][odd]),
             'inputs_length': torch.max(inputs['inputs_length'][even], inputs['inputs_length'][odd])}
    loss_1, _ = model(mixed, {k: v[even] for k, v in targets.items()})
    loss_2, _ = model(mixed, {k: v[odd] for k, v in targets.items()})
    return lam, loss_1, loss_2, torch.mean(lam * loss_1 + (1 - lam) * loss_2)


def main():
    out = {'seed': np.int64(SEED)}
    for tag, ctc_weight in (('att', 0.0), ('joint', 0.3)):
        cfg = syn.c1_model(0.0, ctc_weight=ctc_weight)
        torch.manual_seed(1234)
        model = End2EndModel[cfg['type']](cfg)
        syn.fill_state_dict_(model.state_dict(), 1234)
        model.train()
        inputs, targets = syn.synthetic_batch(**BATCH)
        np.random.seed(SEED)
        lam, loss_1, loss_2, loss = mixspeech_step(model, inputs, targets)
        loss.backward()
        keys, vals = [], []
        for k, p in model.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.detach().double().reshape(-1).numpy()
            keys.append(k)
            vals.append([np.sqrt((g * g).sum()), float((g * probe_vector(k, g.size)).sum())])
        out.update({tag + '_lambda': lam.numpy(), tag + '_loss_1': np.float64(loss_1.item()), tag + '_loss_2': np.float64(loss_2.item()),
                    tag + '_loss': np.float64(loss.item()), tag + '_grad_keys': np.array(keys),
                    tag + '_grad_summary': np.array(vals, dtype=np.float64)})
        print(tag, 'lambda', float(lam), 'loss_1', loss_1.item(), 'loss_2', loss_2.item(), 'loss', loss.item(), len(keys), 'gradients')
    path = os.path.join(HERE, 'golden', 'mixspeech_c1.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
