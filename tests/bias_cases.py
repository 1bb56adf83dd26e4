"""The recognizer case of the phrase-biasing tests (tests/test_gpu_bias.py), modelled on tests/ngram_attn_cases.py and built on it: the
C1 model with a CTC head, V = 100, its batch of 4 with the 13-frame utterance, beam 5, n-best 3, max_len 10, the 2-block
TransformerLM -- and the restatement of its searches (tests/bias_ref.py) on the oracle's decoder, CTC head and LM over a given
encoder memory.  With the oracle's encoder in the memory's place (oracle_memory) the same function runs without a GPU, which is how
the phrase sets below were chosen, per (mode, with / without the n-gram of ngram_attn_cases):
 (a) at every step the restatement's gap between the last kept and the first dropped entry (pre-beam cut, per-row cut, beam^2 prune,
     n-best) exceeds GAP, so f32 noise cannot change a token;
 (b) the biased 1-best differs from the unbiased one for at least one utterance.
The first phrase of every set is the unbiased SECOND-best hypothesis of one utterance, with a per-token weight above the score gap
to the best divided by its length; the others are there to be walked into and left again (refunds), and share prefixes with it.
The GPU test asserts (a) on its own memory and (b) on its own result."""
from tests import bias_ref as ref
from tests import ngram_attn_cases as base
from tests.ngram_attn_cases import (BEAM, BLANK, EOS, GAP, INPUT_SEED, LAMBDA, LM_CFG, LM_WEIGHT, MAX_LEN, MODES, NBEST, V,   # noqa: F401
                                    batch, model_cfg, ngram, oracle_memory)
from oracle import otrans_oracle as orc

# (mode, with the n-gram) -> (phrases, per-token weights)
_LONG_A = (28, 32, 6, 9, 3, 19, 81, 65, 91, 51, 61, 97, 73, 63, 55, 56)
_LONG_B = (85, 8, 81, 94, 27, 18, 9, 80, 94, 61, 62, 79, 2, 83, 91, 14)
PHRASES = {
    ('plain', False): ([(85,) * 10, (85, 85, 85, 85), (64, 85), (52,), _LONG_A, (85, 29, 81)], [1.35, 0.5, 1.0, 0.75, 0.25, 1.5]),
    ('plain', True): ([(64,) * 10, (64, 64, 64, 85), (64, 64), (52,), _LONG_A, (64, 29, 81)], [0.25, 0.5, 1.0, 0.75, 0.25, 1.5]),
    ('joint', False): ([(3, 3), (3, 3, 85), (64, 3), (52,), _LONG_A, (3, 29, 81)], [6.45, 0.5, 1.0, 0.75, 0.25, 1.5]),
    ('joint', True): ([(36,) * 10, (36, 36, 36, 89), (86, 36), (82,), _LONG_B, (36, 85, 30)], [0.15, 0.5, 1.0, 0.75, 0.25, 1.5]),
}


def phrase_set(mode, with_ngram):
    """(PhraseBias, RefBias) of a case"""
    from opentransformer_amd.bias import PhraseBias
    phrases, weights = PHRASES[(mode, bool(with_ngram))]
    return PhraseBias(phrases, V, weights=weights, eos_unit=EOS), ref.RefBias(phrases, weights, V, EOS)


def restated(cfg, sd, lm_sd, mem, mm, mode, bias, ng=None, alpha=0.0, beta=0.0, beam=BEAM, max_len=MAX_LEN, nbest=NBEST, K=None):
    """the restated search over encoder memory `mem` / mask `mm` (CPU, f32): mode 'plain' or 'joint'; bias a RefBias, or None for
    the search without phrases (a RefBias of one phrase at weight 0 adds +0.0, which changes no f32 value); ng a RefLM with its
    alpha / beta, or None.  Returns (hyps, scores, gaps)."""
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
    if bias is None:
        bias = ref.RefBias([(2,)], [0.0], V, EOS)
    gaps = []
    hyps, scores = ref.beam_search(att, B, beam, max_len, EOS, dict(ref=bias, K=K),
                                   ngram=dict(lm=ng, alpha=alpha, beta=beta, K=K) if ng is not None else None, lm_fn=lm_fn,
                                   lm_weight=LM_WEIGHT if lm_sd is not None else 0.0, joint=joint, nbest=nbest, gaps=gaps)
    return hyps, scores, gaps
