"""The inputs of the device comparisons of the LM-fused CTC prefix beam search (tests/test_gpu_ctc_ngram.py), shared with the CPU
test that asserts, on the restatement alone, that each of them leaves at least three quarters of its utterances clear of a W/W+1
near-tie: the GPU tests' `min_clear` then cannot hide a failure.  The restatement of a case is computed once per process."""
import functools
import os

import numpy as np

from opentransformer_amd.ngram import NGramLM
from tests import ctc_prefix_lm_ref as lmref
from tests.ngram_ref import RefLM, make_lm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ALPHA, BETA, GAP = 0.5, 1.0, 1e-4
GOLDEN_LENGTHS = ([35, 35, 35, 35], [35, 30, 17, 1])
GOLDEN_WS, GOLDEN_KS, GOLDEN_ORDERS = (1, 5, 32), (5, 40, 100), (1, 3)
SIZE_LENGTHS = [0, 1, 300, 200, 64, 299]


@functools.lru_cache(maxsize=None)
def lm_pair(seed, V, order, per_order, absent=(), unk_unit=None, tight=True):
    """(NGramLM loaded from the generated ARPA text, RefLM over the same values)"""
    import io
    text, grams, idx2unit = make_lm(seed, V, order, list(per_order), absent=absent, unk_unit=unk_unit)
    lm = NGramLM.from_arpa(io.StringIO(text), idx2unit, unk_unit=unk_unit)
    if not tight:
        lm = NGramLM.from_arpa(io.StringIO(text), idx2unit, unk_unit=unk_unit, capacity=4 * lm.capacity)
    return lm, RefLM(grams, order, V, lm.oov_score)


def golden_lm(order):
    """the LM of the golden-input comparisons: V = 100, units 0 (blank), 7 and 63 left out"""
    return lm_pair(5, 100, order, (600, 900)[:order - 1], absent=(7, 63), unk_unit=2)


@functools.lru_cache(maxsize=None)
def golden_log_probs():
    return np.load(os.path.join(GOLDEN, 'c1_decode.npz'))['ctc_head_logp'].astype(np.float32)        # [4, 35, 100]


@functools.lru_cache(maxsize=None)
def golden_reference(W, K, order, which):
    """(tokens, out_len, scores, lm_scores, gaps) of the restatement on the golden log-probs with GOLDEN_LENGTHS[which]"""
    gaps = []
    out = lmref.decode(golden_log_probs(), GOLDEN_LENGTHS[which], W, K, golden_lm(order)[1], ALPHA, BETA, min_gap=gaps)
    return out + (gaps,)


def size_lm():
    """about 20 k n-grams of order 3 over V = 4233; blank and every 50th unit are left out"""
    return lm_pair(3, 4233, 3, (8000, 8000), absent=tuple(range(50, 4233, 50)))


@functools.lru_cache(maxsize=None)
def size_log_probs():
    import torch
    rng = np.random.default_rng(23)
    x = torch.from_numpy(rng.normal(size=(6, 300, 4233)).astype(np.float32) * 4.0)
    return torch.log_softmax(x, -1).numpy()


@functools.lru_cache(maxsize=None)
def size_reference():
    gaps = []
    out = lmref.decode(size_log_probs(), SIZE_LENGTHS, 10, 40, size_lm()[1], ALPHA, BETA, min_gap=gaps)
    return out + (gaps,)


def clear_count(gaps):
    return sum(g > GAP for g in gaps)
