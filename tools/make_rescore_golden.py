#!/usr/bin/env python3
"""Generate tests/golden/c1_rescore.npz by running the REAL reference's decoder and language model, on the CPU, over the CTC n-best
of the c1_decode.npz fixture: what pins tests/rescore_ref.py (through the oracle) and the HIP path's two-pass decode.

    python tools/make_rescore_golden.py --reference /path/to/OpenTransformer

Setup: the trained C1 model and inputs of tests/golden/c1_decode.npz, the seeded TransformerLM of oracle/make_golden.py:golden_decode.
Hypotheses: the W = 5, K = 40 n-best of tests/ctc_prefix_ref.decode on the fixture's 'ctc_head_logp' (the reference's own CTC head).
Per hypothesis h: att(h) / lm(h) = sum_l log_softmax(model.decoder([BOS] + h, memory_b, mask_b))[l, (h + [EOS])[l]] / the same over
lm.predict([BOS] + h, last_frame=False); then the totals and the final order for ctc_weight in {0.3, 0.7} x lm_weight in {0, 0.3}
(tests/rescore_ref.total / order).  The fixture holds data only (a few KB)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, K, MAX_LEN, BOS, EOS = 5, 40, 12, 1, 1
WEIGHTS = [(0.3, 0.0), (0.3, 0.3), (0.7, 0.0), (0.7, 0.3)]      # (ctc_weight, lm_weight)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project (the directory that holds otrans/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'c1_rescore.npz'))
    args = ap.parse_args(argv)
    # second entry only satisfies the bare `from activation import Swish` at otrans/module/ffn.py:9
    sys.path[:0] = [args.reference, os.path.join(args.reference, 'otrans', 'module')]
    from otrans.model import End2EndModel, LanguageModel
    from opentransformer_amd import synthetic as syn
    from tests import ctc_prefix_ref, rescore_ref as ref

    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c1_decode.npz'))
    cfg = syn.c1_model(residual_dropout=0.0, ctc_weight=0.3)
    torch.manual_seed(1234)
    model = End2EndModel[cfg['type']](cfg)
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    model.eval()
    V = cfg['decoder']['vocab_size']
    lm_cfg = syn.lm_config(V, d_model=cfg['decoder']['d_model'], d_ff=128, num_blocks=2)
    torch.manual_seed(7)
    lm = LanguageModel['transformer_lm'](lm_cfg)
    syn.fill_state_dict_(lm.state_dict(), 4321)
    lm.eval()
    with torch.no_grad():
        fe, fm, _ = model.frontend.inference(torch.from_numpy(g['inputs']), torch.from_numpy(g['mask']), None)
        mem, mm, _ = model.encoder(fe, fm)
    lengths = mm.sum(-1).tolist()
    tokens, out_len, scores = ctc_prefix_ref.decode(g['ctc_head_logp'], lengths, W, K)
    B = tokens.shape[0]
    att, lms = np.full((B, W), -np.inf), np.full((B, W), -np.inf)
    with torch.no_grad():
        for b in range(B):
            for w in range(W):
                n = int(out_len[b, w])
                if not (scores[b, w] > -np.inf and n + 1 <= MAX_LEN):
                    continue
                h = tokens[b, w, :n].tolist()
                ys_in, tgt = torch.tensor([[BOS] + h]), h + [EOS]
                logits, _ = model.decoder(ys_in, mem[b:b + 1], mm[b:b + 1])
                lp = torch.log_softmax(logits[0].double(), -1)
                att[b, w] = float(sum(lp[l, t] for l, t in enumerate(tgt)))
                llp = lm.predict(ys_in, last_frame=False)[0].double()
                lms[b, w] = float(sum(llp[l, t] for l, t in enumerate(tgt)))
    out = {'tokens': tokens, 'out_len': out_len, 'scores': scores, 'att': att, 'lm': lms, 'weights': np.array(WEIGHTS),
           'max_len': np.array(MAX_LEN), 'W': np.array(W), 'K': np.array(K)}
    for i, (lam, mu) in enumerate(WEIGHTS):
        tot = np.full((B, W), -np.inf)
        for b in range(B):
            for w in range(W):
                if att[b, w] > -np.inf:
                    tot[b, w] = ref.total(att[b, w], scores[b, w], lms[b, w] if mu else None, lam, mu, int(out_len[b, w]))
        out['total_%d' % i] = tot
        out['perm_%d' % i] = np.array([ref.order(tot[b].tolist()) for b in range(B)], np.int32)
        gaps = [min((abs(x - y) for j, x in enumerate(tot[b]) for y in tot[b][j + 1:] if x > -np.inf and y > -np.inf), default=np.inf)
                for b in range(B)]
        print('ctc_weight %.1f lm_weight %.1f: order %s, smallest gap between two totals per utterance %s'
              % (lam, mu, out['perm_%d' % i].tolist(), ['%.3g' % x for x in gaps]))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
