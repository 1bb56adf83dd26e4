"""MixSpeech restated on the host (otrans/train/trainer.py:155-201), no GPU: what tests/test_mixspeech.py checks on the CPU and
tests/test_gpu_mixspeech.py judges the kernels by.

mix_pairs is the float32 numpy form of trainer.py:172-182 with the rounding order otr_mixspeech_mix documents: 1 - lam rounded once,
each product rounded, then the sum.  ctc_pair composes the paired CTC term from tests/ctc_loss_cases.py's float64 reference (and its
float32 twin, the floor).  rolled() turns a named CTC case into a pair: set a is the case's labels, set b the same rows rolled by one
utterance, in_len shared."""
import functools

import numpy as np
import torch

from tests import ctc_loss_cases as cc


def mix_pairs(x, lengths, lam):
    """(out f32 [P, T, F], out_lengths int32 [P], out_mask bool [P, T]) of x f32 [B, T, F], lengths [B] and a float32 lam; frames at or
    past an utterance's length count as zero whatever x holds there, frames at or past the pair's length are zero"""
    x = np.asarray(x, np.float32)
    B, T, F = x.shape
    P = B // 2
    n = np.clip(np.asarray(lengths, np.int64), 0, T)
    live = np.arange(T)[None, :] < n[:, None]
    z = np.where(live[:, :, None], x, np.float32(0))
    lam = np.float32(lam)
    om = np.float32(1) - lam
    out = (lam * z[0:2 * P:2]).astype(np.float32) + (om * z[1:2 * P:2]).astype(np.float32)
    out_len = np.maximum(n[0:2 * P:2], n[1:2 * P:2]).astype(np.int32)
    mask = np.arange(T)[None, :] < out_len[:, None]
    return np.where(mask[:, :, None], out, np.float32(0)).astype(np.float32), out_len, mask


def rolled(case):
    """(case_a, case_b): case_b is `case` with targets, tgt_len and what it claims per utterance rolled by one (utterance p of b is
    utterance p - 1 of the case); logits and in_len are shared.  raised_tgt_len rolls with the labels, raised_in_len does not apply to
    set b (it belongs to the frames)."""
    b = dict(case, name=case['name'] + '_rolled', targets=torch.roll(case['targets'], 1, 0), tgt_len=torch.roll(case['tgt_len'], 1, 0))
    if case.get('raised_tgt_len') is not None:
        b['raised_tgt_len'] = torch.roll(case['raised_tgt_len'], 1, 0)
    return case, b


@functools.lru_cache(maxsize=None)
def pair_of(name):
    return rolled(cc.build(name))


def ctc_pair(logits, case_a, case_b, lam, dtype):
    """lam * CTC(a) + (1 - lam) * CTC(b) on `logits` in `dtype` (float64: the reference, float32: the floor), each term
    F.log_softmax + F.ctc_loss ('mean', zero_infinity) as tests/ctc_loss_cases.py calls them.  Returns a dict: loss, loss_a, loss_b
    (0-d), nll [2, P], grad [P, T, V] = lam * g_a + (1 - lam) * g_b, and g_a, g_b."""
    return _combine(_terms(logits, case_a, case_b, dtype), lam, dtype)


def _terms(logits, case_a, case_b, dtype):
    """the two sets' (loss, nll, gradient): they do not depend on lam"""
    return (cc._ctc(logits, case_a['targets'], case_a['in_len'], case_a['tgt_len'], case_a['blank'], dtype)
            + cc._ctc(logits, case_b['targets'], case_b['in_len'], case_b['tgt_len'], case_b['blank'], dtype))


def _combine(terms, lam, dtype):
    la, na, ga, lb, nb, gb = terms
    lam = torch.tensor(float(np.float32(lam)), dtype=dtype)
    om = torch.tensor(float(np.float32(1) - np.float32(lam)), dtype=dtype)
    return {'loss': lam * la + om * lb, 'loss_a': la, 'loss_b': lb, 'nll': torch.stack((na, nb)), 'grad': lam * ga + om * gb,
            'g_a': ga, 'g_b': gb}


@functools.lru_cache(maxsize=None)
def _terms_of(name, dtype):
    a, b = pair_of(name)
    return _terms(a['logits'], a, b, dtype)


@functools.lru_cache(maxsize=None)
def reference_of(name, lam):
    return _combine(_terms_of(name, torch.float64), lam, torch.float64)


@functools.lru_cache(maxsize=None)
def floor_of(name, lam):
    """the float32 composition's distance from float64, in the measures tests/test_gpu_ctc_loss.py uses: per utterance 'nll' [2, P]
    (nll_rel), 'grad' [P] (slab_rel of the mixed gradient), and the three losses relative"""
    r64, r32 = reference_of(name, lam), _combine(_terms_of(name, torch.float32), lam, torch.float32)
    rel = lambda k: float((r32[k].double() - r64[k]).abs() / r64[k].abs().clamp_min(1e-300))    # noqa: E731
    return {'nll': torch.stack([cc.nll_rel(r32['nll'][k], r64['nll'][k]) for k in (0, 1)]), 'grad': cc.slab_rel(r32['grad'], r64['grad']),
            'loss': rel('loss'), 'loss_a': rel('loss_a'), 'loss_b': rel('loss_b')}


def pair_coef(case_a, case_b, lam):
    """float64 [P]: lam * ok_a * coef_a + (1 - lam) * ok_b * coef_b, the factor of the softmax in an utterance's mixed gradient; frame
    column sums are judged relative to it"""
    P = case_a['logits'].shape[0]
    lam = float(np.float32(lam))
    om = float(np.float32(1) - np.float32(lam))
    fa = torch.tensor(cc.feasible(case_a), dtype=torch.float64)
    fb = torch.tensor(cc.feasible(case_b), dtype=torch.float64)
    return lam * fa * cc.coef(case_a['tgt_len'], case_a['targets'], P) + om * fb * cc.coef(case_b['tgt_len'], case_b['targets'], P)


# ------------------------------------------------------------------------------------------ the whole step, by the CPU oracle
def oracle_model_loss(parts, cfg, inputs, targets, kind):
    """one plain forward of the oracle: SpeechToText ('att', 'joint') or, kind 'ctc', CTCModel.forward (model/ctc.py:69-96: frontend,
    encoder, the head's CTC loss on the labels truth[:, 1:-1] with lengths targets_length - 1) composed from the oracle's parts"""
    from oracle import otrans_oracle as orc
    if kind != 'ctc':
        return orc.speech2text_forward(parts, cfg, inputs, targets)[0]
    x, mask = orc.conv_frontend(parts['frontend'], inputs['inputs'], inputs['mask'])
    memory, memory_mask = orc.transformer_encoder(parts['encoder'], x, mask, cfg['encoder'])
    logits = torch.nn.functional.linear(memory, parts['ctc']['output_layer.weight'], parts['ctc']['output_layer.bias'])
    truth = targets['targets']
    return orc.ctc_loss(logits, memory_mask.sum(-1), truth[:, 1:-1], targets['targets_length'] - 1)


def oracle_composite(cfg, inputs, targets, lam, seed=1234, kind=None):
    """(loss, loss_1, loss_2, parts) on the CPU: lam * oracle(mixed, t1) + (1 - lam) * oracle(mixed, t2), the mixed batch from mix_pairs,
    the weights those of the project's fill for `seed`; parts' tensors require gradients"""
    from tests import helpers as H
    kind = kind or ('joint' if cfg.get('ctc_weight', 0.0) > 0 else 'att')
    parts = H.require_grad(H.filled_state(cfg, seed=seed, with_ctc=True if kind == 'ctc' else None))
    if kind == 'ctc':
        parts.pop('decoder')
    x, n, mask = mix_pairs(inputs['inputs'].numpy(), inputs['inputs_length'].numpy(), lam)
    mixed = {'inputs': torch.from_numpy(x), 'mask': torch.from_numpy(mask), 'inputs_length': torch.from_numpy(n)}
    B = inputs['inputs'].shape[0] // 2 * 2
    losses = [oracle_model_loss(parts, cfg, mixed, {k: v[i:B:2] for k, v in targets.items()}, kind) for i in (0, 1)]
    lam = float(np.float32(lam))
    om = float(np.float32(1) - np.float32(lam))
    return lam * losses[0] + om * losses[1], losses[0], losses[1], parts
