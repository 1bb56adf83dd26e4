"""Error-rate scoring on the device: the WER / top-n WER bookkeeping of the reference's decode loop (eval.py:121-202) and of
tools/computer_wer.py, on ops.edit_distance (csrc/editdist.hip) instead of the `editdistance` package.

The hypotheses of every search here already live on the device (recognize_tokens of both recognizers), so a pass over a dev set is
one launch per batch that also adds the corpus totals into an int64 [8] tensor, and ONE copy to the host at the end:

    meter = ErrorRateMeter(device)
    result = evaluate(recognizer, loader, meter)        # {'wer': ..., 'topn_wer': ..., 'errors': ..., ...}

Units are whatever the token ids stand for: characters give CER, words WER.  score_texts scores word lists (two files of
`utt_id word word ...` lines in tools/compute_wer.py) by mapping words to ids on the host first."""
import math

import torch

from . import ops
from .nn import EOS

_FIELDS = ('utterances', 'ref_tokens', 'errors', 'substitutions', 'deletions', 'insertions', 'errors_oracle', 'bad')


def result_from_totals(totals):
    """the result dict of eight totals (include/otrans_hip.h otr_edit_distance; any sequence of 8 ints): wer and topn_wer in percent as
    eval.py:190-193 computes them (1-best errors, and the least errors over each utterance's n-best, over the reference tokens; nan
    where there are no reference tokens), and the counts"""
    t = dict(zip(_FIELDS, (int(v) for v in totals)))
    n = t['ref_tokens']
    out = {'wer': t['errors'] / n * 100 if n else float('nan'), 'topn_wer': t['errors_oracle'] / n * 100 if n else float('nan')}
    out.update(t)
    return out


class ErrorRateMeter:
    """Corpus totals of ops.edit_distance on `device`.  update() launches and never synchronises; result() is the one copy to the
    host.  An utterance whose reference or first hypothesis has a length outside its tensor counts under 'bad' and nowhere else."""

    def __init__(self, device):
        self.totals = torch.zeros(8, dtype=torch.int64, device=device)

    def update(self, ref, ref_len, hyp, hyp_len=None, eos=-1):
        """ref [B, Lr], ref_len [B], hyp [B, N, Lh] or [B, Lh], hyp_len [B, N] or None (the full width), as ops.edit_distance takes
        them.  Returns (dist int32 [B, N], counts int32 [B, N, 3]) on the device."""
        dist, counts, _ = ops.edit_distance(ref, ref_len, hyp, hyp_len, eos=eos, totals=self.totals)
        return dist, counts

    def result(self):
        return result_from_totals(self.totals.cpu().tolist())

    def reset(self):
        self.totals.zero_()


def calibration(conf, correct, mask=None, eps=1e-6, bins=10):
    """How well confidences predict outcomes: conf in [0, 1] and correct (bool or 0 / 1) device tensors of one shape, mask (bool, None:
    all) the elements that count.  Returns {'nce', 'ece', 'tokens'}.  NCE, the normalised cross-entropy, is (H_prior - H_conf) /
    H_prior: H_prior the entropy of the outcomes at their mean rate, H_conf the cross-entropy of the confidences (clamped to [eps,
    1 - eps]); 1 is perfect, 0 no better than quoting the mean rate, negative worse; nan where every outcome is the same.  ECE, the
    expected calibration error, is the sum over `bins` equal-width bins of n_k / n * |mean outcome - mean confidence|.  A few float64
    reductions on the device and one read by the host."""
    c = conf.reshape(-1).double()
    y = correct.reshape(-1).double()
    w = torch.ones_like(c) if mask is None else mask.reshape(-1).double()
    cc = c.clamp(eps, 1.0 - eps)
    hc = -(w * (y * torch.log(cc) + (1.0 - y) * torch.log1p(-cc))).sum()
    k = (c * bins).long().clamp_(0, bins - 1)
    zero = torch.zeros(bins, dtype=torch.float64, device=c.device)
    gap = (zero.index_add(0, k, w * y) - zero.index_add(0, k, w * c)).abs().sum()
    n, nc, hc, gap = torch.stack((w.sum(), (w * y).sum(), hc, gap)).tolist()
    if n == 0:
        return {'nce': float('nan'), 'ece': float('nan'), 'tokens': 0}
    hp = -(nc * math.log(nc / n) + (n - nc) * math.log(1.0 - nc / n)) if 0 < nc < n else 0.0
    return {'nce': (hp - hc) / hp if hp > 0 else float('nan'), 'ece': gap / n, 'tokens': int(n)}


@torch.no_grad()
def evaluate(recognizer, batches, meter=None, confidence=False):
    """The decode-and-score loop of eval.py:126-193.  `batches` yields (utt_id, inputs, targets) as data.collate_fn_with_eos_bos
    builds them, on the recognizer's device.  The reference tokens are targets['targets'][:, 1:] with length targets_length - 1
    (eval.py:149: without BOS, without EOS); the hypotheses are recognizer.recognize_tokens(...), cut before their first EOS as
    translate / nbest_translate cut the strings.  Nothing is copied to the host per batch by this loop; returns meter.result().
    confidence=True: the hypotheses come from recognizer.recognize_tokens_with_confidence(...), a token of the 1-best counts as
    correct where ops.edit_align against the reference calls it a match, and the result gains 'nce' and 'ece' (calibration() over all
    the 1-best tokens of the pass, still one read at the end)."""
    kept = []
    for _, inputs, targets in batches:
        ref, ref_len = targets['targets'][:, 1:], targets['targets_length'] - 1
        if confidence:
            tokens, lengths, _, conf, _ = recognizer.recognize_tokens_with_confidence(inputs['inputs'], inputs['mask'])
            W = ops.NBEST_MAX_LEN                         # a longer 1-best or reference is an invalid pair there: left out of nce / ece
            code = ops.edit_align(ref[:, :W], ref_len, tokens[:, :1, :W], lengths[:, :1], eos=EOS)[1][:, 0]
            kept.append((conf[:, :W].reshape(-1), (code == 0).reshape(-1), (code >= 0).reshape(-1)))
        else:
            tokens, lengths, _ = recognizer.recognize_tokens(inputs['inputs'], inputs['mask'])
        if meter is None:
            meter = ErrorRateMeter(tokens.device)
        meter.update(ref, ref_len, tokens, lengths, eos=EOS)
    if meter is None:
        raise ValueError('evaluate: no batches and no meter')
    out = meter.result()
    if confidence:
        cal = calibration(*(torch.cat(t) for t in zip(*kept)))
        out['nce'], out['ece'] = cal['nce'], cal['ece']
    return out


def texts_to_ids(refs, hyps):
    """Host side of score_texts: two dicts utt_id -> list of words (or two equally long lists of word lists) -> (ref int64 [B, Lr]
    padded with 0, ref_len int32 [B], hyp int64 [B, Lh], hyp_len int32 [B], ids: the utterances in scoring order, unmatched: the ids
    of `hyps` that `refs` lacks).  Words are numbered from 1 in order of first appearance, references first.  The utterances are the
    hypotheses' that have a reference, in the hypotheses' order, as computer_wer.py walks its predict file."""
    if isinstance(refs, dict) != isinstance(hyps, dict):
        raise TypeError('score_texts: refs and hyps must both be dicts or both be lists')
    if isinstance(refs, dict):
        ids = [u for u in hyps if u in refs]
        unmatched = [u for u in hyps if u not in refs]
        pairs = [(refs[u], hyps[u]) for u in ids]
    else:
        if len(refs) != len(hyps):
            raise ValueError('score_texts: %d references and %d hypotheses' % (len(refs), len(hyps)))
        ids, unmatched, pairs = list(range(len(refs))), [], list(zip(refs, hyps))
    vocab = {}
    rows = [([vocab.setdefault(w, len(vocab) + 1) for w in r], h) for r, h in pairs]
    rows = [(r, [vocab.setdefault(w, len(vocab) + 1) for w in h]) for r, h in rows]
    B = len(rows)
    Lr, Lh = max([len(r) for r, _ in rows] + [1]), max([len(h) for _, h in rows] + [1])
    ref, hyp = torch.zeros((B, Lr), dtype=torch.int64), torch.zeros((B, Lh), dtype=torch.int64)
    for b, (r, h) in enumerate(rows):
        ref[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
        hyp[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
    ref_len = torch.tensor([len(r) for r, _ in rows], dtype=torch.int32)
    hyp_len = torch.tensor([len(h) for _, h in rows], dtype=torch.int32)
    return ref, ref_len, hyp, hyp_len, ids, unmatched


def score_texts(refs, hyps, device='cuda'):
    """Score word lists on the device: refs / hyps are dicts utt_id -> list of words, or two lists.  An id of `hyps` that `refs` lacks
    is skipped and returned under 'unmatched'.  Returns ErrorRateMeter.result()'s dict plus 'unmatched'.  Utterances longer than
    ops.EDIT_MAX_LEN words raise ValueError."""
    ref, ref_len, hyp, hyp_len, _, unmatched = texts_to_ids(refs, hyps)
    meter = ErrorRateMeter(device)
    if ref.size(0):
        meter.update(ref.to(device), ref_len.to(device), hyp.to(device), hyp_len.to(device))
    out = meter.result()
    out['unmatched'] = unmatched
    return out
