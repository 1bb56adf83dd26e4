"""The recognizer case of the n-gram fusion tests (tests/test_gpu_ngram_attn.py): the C1 model with a CTC head, V = 100, batch 4 with
the 13-frame utterance, a 2-block TransformerLM and an order-3 n-gram over the 100 units -- and the restatement of its searches
(tests/ngram_attn_ref.py) on the oracle's decoder, CTC head and LM over a given encoder memory.  The memory is the only input that
comes from the device; with the oracle's encoder in its place the same function runs without a GPU, which is how the seeds below
were chosen: at every step the restatement's gap between the last kept and the first dropped entry (pre-beam cut, per-row cut,
beam^2 prune, n-best) exceeds GAP, so f32 noise cannot change a token.  The GPU test asserts that gap on its own memory."""
import torch

from opentransformer_amd import synthetic as syn
from oracle import otrans_oracle as orc
from tests import ngram_attn_ref as ref
from tests.ngram_cases import lm_pair

BLANK, EOS, V = 0, 1, 100
GAP = 1e-4
BEAM, NBEST, MAX_LEN, LM_WEIGHT, LAMBDA = 5, 3, 10, 0.3, 0.3
INPUT_SEED = 11
# per mode: the n-gram's seed and weights.  Plain: a length bonus large enough that the hypotheses do not end at once (the synthetic
# decoder is nearly flat); joint: the CTC head ends them.  Chosen on the CPU for their gaps (see above).
MODES = {'plain': dict(lm_seed=5, alpha=0.5, beta=2.5), 'joint': dict(lm_seed=6, alpha=0.5, beta=1.0)}
LM_CFG = syn.lm_config(100, d_model=64, d_ff=128, num_blocks=2)


def model_cfg():
    return syn.c1_model(0.0, ctc_weight=0.3)


def batch(seed=INPUT_SEED):
    inputs, _ = syn.synthetic_batch(batch=4, frames=120, feat_dim=80, vocab=100, tgt_len=6, seed=seed, lengths=[120, 96, 13, 70],
                                    tgt_lengths=[6, 6, 6, 6])
    return inputs['inputs'], inputs['mask']


def ngram(seed):
    """(NGramLM, RefLM): order 3 over the 100 units (make_lm leaves the blank out)"""
    return lm_pair(seed, V, 3, (600, 900))


def restated(cfg, sd, lm_sd, mem, mm, mode, ng, alpha, beta, beam=BEAM, max_len=MAX_LEN, nbest=NBEST, K=None):
    """the restated search over encoder memory `mem` / mask `mm` (CPU, f32): mode 'plain' or 'joint'; sd the model's state dict,
    lm_sd the TransformerLM's (or None).  Returns (hyps, scores, gaps)."""
    dec = {k[8:]: v for k, v in sd.items() if k.startswith('decoder.')}
    ctc = {k[9:]: v for k, v in sd.items() if k.startswith('assistor.')}
    B, T, D = mem.shape
    bm = mem.unsqueeze(1).repeat(1, beam, 1, 1).view(B * beam, T, D)
    bmask = mm.unsqueeze(1).repeat(1, beam, 1).view(B * beam, T)
    att = lambda p: orc.decoder_inference(dec, p, bm, bmask, cfg['decoder'])          # noqa: E731
    lm_fn = (lambda p: orc.lm_step_log_probs((lm_sd, LM_CFG), p)) if lm_sd is not None else None     # noqa: E731
    K = K or min(V, int(1.5 * beam))
    joint = None
    if mode == 'joint':
        clp, cln = orc.ctc_inference(ctc, mem, mm)
        joint = dict(x=clp.double().tolist(), lengths=cln.tolist(), ctc_weight=LAMBDA, K=K, blank=BLANK)
    gaps = []
    hyps, scores = ref.beam_search(att, B, beam, max_len, EOS, dict(lm=ng, alpha=alpha, beta=beta, K=K), lm_fn=lm_fn,
                                   lm_weight=LM_WEIGHT if lm_sd is not None else 0.0, joint=joint, nbest=nbest, gaps=gaps)
    return hyps, scores, gaps


def oracle_memory(cfg, sd, x, m):
    """the encoder memory from the oracle's frontend and encoder: what the device computes, to f32 rounding"""
    fe = {k[9:]: v for k, v in sd.items() if k.startswith('frontend.')}
    enc = {k[8:]: v for k, v in sd.items() if k.startswith('encoder.')}
    with torch.no_grad():
        y, mask = orc.conv_frontend(fe, x, m)
        return orc.transformer_encoder(enc, y, mask, cfg['encoder'])
