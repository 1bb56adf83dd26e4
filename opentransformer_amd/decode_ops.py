"""No-autograd wrappers over the C ABI (include/otrans_hip.h) for search, scoring, alignment and evaluation.  The rules are those of
ops.py: raw data_ptr()s and torch's current stream go to libotrans_hip.so, a non-CUDA tensor raises.  ops.py re-exports every public
name below, and `ops.X` is how the package, the tests and the tools call them."""
import math

import torch

from . import _lib as L
from ._runtime import _cuda, _p, _stream, _timed

__all__ = ['log_softmax', 'ctc_prefix_beam_search', 'ctc_prefix_beam_search_lm', 'ctc_prefix_beam_search_bias', 'ngram_lookup',
           'ngram_score_candidates', 'ngram_score_sequences', 'bias_score_candidates', 'bias_score_sequences', 'ctc_forced_align',
           'ctc_segment', 'edit_distance', 'edit_align', 'nbest_consensus', 'joint_prebeam', 'ctc_prefix_score', 'rescore_pack',
           'attention_rescore', 'CTC_ALIGN_MAX_TGT', 'CTC_SEGMENT_MAX_TGT', 'EDIT_MAX_LEN', 'EDIT_MAX_NBEST', 'NBEST_MAX_LEN',
           'JOINT_MAX_K', 'JOINT_MAX_T', 'JOINT_MAX_V', 'JOINT_MAX_BEAM', 'RESCORE_MAX_W', 'RESCORE_MAX_V']


def log_softmax(x):
    """F.log_softmax(x, -1) for fp32 x (no autograd; decode / CTC inference paths)."""
    _cuda(x)
    V = x.shape[-1]
    x2 = x.reshape(-1, V).contiguous().float()
    y = torch.empty_like(x2)
    L.check(L.load().otr_log_softmax(_p(x2), _p(y), x2.shape[0], V, _stream()), 'otr_log_softmax')
    return y.view(x.shape)


def ctc_prefix_beam_search(log_probs, lengths, beam_width=5, cutoff_top_n=40, blank=0, workspace=None):
    """CTC prefix beam search on the device (include/otrans_hip.h otr_ctc_topk + otr_ctc_beam_search; the decoder that
    recognize/ctc.py:60-67 takes from ctcdecode.CTCBeamDecoder without a scorer).  log_probs f32 [B, T, V] (log-softmax output),
    lengths [B] frames per utterance.  Returns (tokens int64 [B, W, T] padded with -1, out_len int32 [B, W], scores f32 [B, W]),
    each utterance's beam in descending score order; slots past the live beam have score -inf and length 0.  cutoff_top_n is
    clamped to V.  ctcdecode's score-threshold pruning (cutoff_prob / "min_cutoff") is not applied.  Two launches on the current
    stream, no host synchronisation: capturable into a graph (pass `workspace`, otr_ctc_beam_workspace_bytes bytes, to reuse one)."""
    return _ctc_prefix_beam_search('ctc_prefix_beam_search', log_probs, lengths, beam_width, cutoff_top_n, blank, workspace, None)


def _ctc_prefix_beam_search(who, log_probs, lengths, beam_width, cutoff_top_n, blank, workspace, lm, bias=None):
    """the argument checks, the buffers and the top-K pass every search shares; lm = None or (NGramLM, alpha, beta); bias = None or a
    bias.PhraseBias (then the phrase-biased entry runs, with the n-gram too where lm is given)"""
    _cuda(log_probs, lengths)
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32:
        raise L.OtransHipError('%s: log_probs must be f32 [B, T, V], got %s %s' % (who, log_probs.dtype, tuple(log_probs.shape)))
    B, T, V = log_probs.shape
    W, K = int(beam_width), min(int(cutoff_top_n), V)
    lib = L.load()
    lp = log_probs if log_probs.stride(2) == 1 and log_probs.stride(0) == T * log_probs.stride(1) else log_probs.contiguous()
    ln = lengths.to(torch.int32).contiguous()
    dev = log_probs.device
    need = lib.otr_ctc_beam_workspace_bytes(B, T, W)
    if need < 0 or not 0 <= blank < V:            # refused before the first launch (the library checks everything again)
        raise L.OtransHipError('%s: bad arguments B=%d T=%d beam_width=%d blank=%d V=%d' % (who, B, T, W, blank, V))
    if lm is not None and lm[0].vocab_size != V:
        raise L.OtransHipError('%s: the n-gram LM was loaded for %d units, log_probs has V=%d' % (who, lm[0].vocab_size, V))
    top_lp = torch.empty((B * T, K), dtype=torch.float32, device=dev)
    top_tok = torch.empty((B * T, K), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)
    tokens = torch.empty((B, W, T), dtype=torch.int64, device=dev)
    out_len = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    L.check(lib.otr_ctc_topk(_p(lp), lp.stride(1), _p(ln), B, T, V, K, _p(top_lp), _p(top_tok), _stream()), 'otr_ctc_topk')
    args = [_p(top_lp), _p(top_tok), _p(ln), B, T, V, K, blank, W, _p(workspace), workspace.numel() * workspace.element_size(),
            _p(tokens), _p(out_len), _p(scores)]
    terms = ()                                    # the score terms returned behind `scores`, in the order of the entry's arguments
    if lm is not None:
        ngram, alpha, beta = lm
        lm_scores = torch.empty((B, W), dtype=torch.float32, device=dev)
        args += [_p(ngram.device_table(dev)), ngram.capacity, ngram.max_probe, ngram.order, float(alpha), float(beta), ngram.oov_score,
                 _p(lm_scores)]
        terms += (lm_scores,)
    elif bias is not None:                        # the biased entry always has the n-gram group: no table, no term
        args += [None, 0, 0, 0, 0.0, 0.0, 0.0, None]
    if bias is not None:
        bias_scores = torch.empty((B, W), dtype=torch.float32, device=dev)
        args += [_p(bias.device_table(dev)), bias.capacity, bias.max_probe, bias.max_len, _p(bias_scores)]
        terms += (bias_scores,)
    entry = 'otr_ctc_beam_search' + ('_bias' if bias is not None else '_lm' if lm is not None else '')
    L.check(getattr(lib, entry)(*args, _stream()), entry)
    return (tokens, out_len, scores) + terms


def ctc_prefix_beam_search_lm(log_probs, lengths, ngram, alpha, beta, beam_width=5, cutoff_top_n=40, blank=0, workspace=None):
    """ctc_prefix_beam_search with a backoff n-gram LM fused into the search (include/otrans_hip.h otr_ctc_beam_search_lm): every
    extension s -> s+c gains alpha * ln P_LM(c | <s> s) + beta, what ctcdecode.CTCBeamDecoder does with a character-based scorer.
    `ngram`: an opentransformer_amd.ngram.NGramLM loaded for the V units of log_probs (uploaded on first use; graph capture wants
    ngram.to(device) called before).  Returns (tokens, out_len, scores, lm_scores f32 [B, W]): scores include the LM term,
    lm_scores is that term alone (scores - lm_scores: the acoustic log-probability).  Same launches, same capturability."""
    return _ctc_prefix_beam_search('ctc_prefix_beam_search_lm', log_probs, lengths, beam_width, cutoff_top_n, blank, workspace,
                                   (ngram, alpha, beta))


def ctc_prefix_beam_search_bias(log_probs, lengths, bias, ngram=None, alpha=0.0, beta=0.0, beam_width=5, cutoff_top_n=40, blank=0,
                                workspace=None):
    """ctc_prefix_beam_search with phrase biasing (hotwords) fused into the search (include/otrans_hip.h otr_ctc_beam_search_bias),
    and the n-gram LM of ctc_prefix_beam_search_lm too where `ngram` is given: every extension s -> s+c gains psi_minus(state(s c)) -
    psi(state(s)) of `bias` (an opentransformer_amd.bias.PhraseBias built for the V units of log_probs, none of its phrases holding
    the blank), behind the n-gram's addend; after the last frame an open match is refunded and the beam ranked again.  Returns
    (tokens, out_len, scores, bias_scores f32 [B, W]) without an n-gram, (tokens, out_len, scores, lm_scores, bias_scores) with one:
    scores include every term, bias_scores is what the completed phrases of the hypothesis earned (ops.bias_score_sequences of it).
    Same two launches, no host synchronisation: capturable (call bias.to(device), and ngram.to(device), before a capture)."""
    from .bias import PhraseBias
    if not isinstance(bias, PhraseBias):
        raise L.OtransHipError('ctc_prefix_beam_search_bias: bias must be an opentransformer_amd.bias.PhraseBias, got %s'
                               % type(bias).__name__)
    V = log_probs.shape[-1]
    if bias.vocab_size != V:
        raise L.OtransHipError('ctc_prefix_beam_search_bias: the phrase set was built for %d units, log_probs has V=%d'
                               % (bias.vocab_size, V))
    held = [p for p in bias.phrases if blank in p]
    if held:            # it could never match (the blank is never emitted): a vocabulary mix-up, not a phrase
        raise L.OtransHipError('ctc_prefix_beam_search_bias: the phrase %r holds the blank id %d' % (held[0], blank))
    return _ctc_prefix_beam_search('ctc_prefix_beam_search_bias', log_probs, lengths, beam_width, cutoff_top_n, blank, workspace,
                                   None if ngram is None else (ngram, alpha, beta), bias)


def ngram_lookup(ngram, ctx, ctx_len, tok):
    """ln P(tok | ctx) of an NGramLM on the device (include/otrans_hip.h otr_ngram_lookup): ctx int32 [n, max(order-1, 1)] rows of
    context ids oldest first, left aligned, ctx_len int32 [n], tok int32 [n] -> f32 [n].  NGramLM.lookup builds these from lists."""
    _cuda(ctx, ctx_len, tok)
    n = tok.numel()
    ctx, ctx_len, tok = ctx.to(torch.int32).contiguous(), ctx_len.to(torch.int32).contiguous(), tok.to(torch.int32).contiguous()
    if ctx_len.numel() != n or ctx.numel() != n * max(ngram.order - 1, 1):
        raise L.OtransHipError('ngram_lookup: ctx %s / ctx_len %s do not match %d tokens at order %d'
                               % (tuple(ctx.shape), tuple(ctx_len.shape), n, ngram.order))
    out = torch.empty(n, dtype=torch.float32, device=tok.device)
    L.check(L.load().otr_ngram_lookup(*_ngram_args(ngram, tok.device), _p(ctx), _p(ctx_len), _p(tok), n, ngram.oov_score, _p(out),
                                      _stream()), 'otr_ngram_lookup')
    return out


def _ngram_args(ngram, dev):
    """the table arguments every n-gram entry takes, in the order of include/otrans_hip.h"""
    return _p(ngram.device_table(dev)), ngram.capacity, ngram.max_probe, ngram.order, ngram.vocab_size


def _score_candidates(who, entry, table_args, table, scalars, preds, cand_idx, cand_score, eos, t, pos, flags, beam, cand_out,
                      with_add, k_score, k_idx):
    """the checks, the buffers and the launch ngram_score_candidates and bias_score_candidates share; table_args(table, device): the
    entry's leading arguments, scalars: what the scorer passes between K and eos"""
    _cuda(preds, cand_idx, cand_score, pos, flags)
    if preds.dtype != torch.int64 or cand_idx.dtype != torch.int32 or cand_score.dtype != torch.float32:
        raise L.OtransHipError('%s: preds int64, cand_idx int32, cand_score f32 expected' % who)
    if preds.dim() != 2 or preds.stride(1) != 1 or cand_idx.shape != cand_score.shape or not cand_idx.is_contiguous() \
            or not cand_score.is_contiguous() or cand_idx.shape[0] != preds.shape[0]:
        raise L.OtransHipError('%s: preds [R, ldp] and contiguous cand_idx / cand_score [R, K] expected, got %s %s %s'
                               % (who, tuple(preds.shape), tuple(cand_idx.shape), tuple(cand_score.shape)))
    R, K = cand_idx.shape
    dev = preds.device
    if cand_out is None:
        cand_out = torch.empty_like(cand_score)
    add = torch.empty_like(cand_score) if with_add else None
    beam = int(beam)
    if beam > 0 and k_score is None:
        k_score = torch.empty((R, beam), dtype=torch.float32, device=dev)
        k_idx = torch.empty((R, beam), dtype=torch.int64, device=dev)
    L.check(getattr(L.load(), entry)(*table_args(table, dev), _p(preds), preds.stride(0), int(t), _p(pos), _p(flags), _p(cand_idx),
                                     _p(cand_score), R, K, *scalars, int(eos), _p(cand_out), _p(add), beam,
                                     _p(k_score) if beam > 0 else None, _p(k_idx) if beam > 0 else None, _stream()), entry)
    return cand_out, add, k_score, k_idx


def ngram_score_candidates(ngram, preds, cand_idx, cand_score, alpha, beta, eos, t=0, pos=None, flags=None, beam=0, cand_out=None,
                           with_add=False, k_score=None, k_idx=None):
    """The n-gram addend of the pre-beam candidates (include/otrans_hip.h otr_ngram_score_cands).  preds int64 [R, ldp]: row r's prefix
    is preds[r, :t] (t = pos + 1 with pos a device int32 scalar, when given), column 0 standing for <s>; cand_idx int32 / cand_score f32
    [R, K'] from joint_prebeam; flags u8 [R] marks finished rows (copied unchanged).  cand_out (default: a new tensor; may be
    cand_score itself) = cand_score + alpha * ln P(c | context) + (c == eos ? 0 : beta).  beam > 0: also the top-`beam` of each row in
    the prune's layout (k_score f32 / k_idx int64 [R, beam]).  Returns (cand_out, cand_add or None, k_score, k_idx).  One launch on the
    current stream, no host synchronisation: capturable (call ngram.to(device) before a capture)."""
    return _score_candidates('ngram_score_candidates', 'otr_ngram_score_cands', _ngram_args, ngram,
                             (float(alpha), float(beta), ngram.oov_score), preds, cand_idx, cand_score, eos, t, pos, flags, beam,
                             cand_out, with_add, k_score, k_idx)


def _score_sequences_args(who, tokens, out_len):
    """the checks and the operands ngram_score_sequences and bias_score_sequences share -> (tokens, lengths, T, out)"""
    _cuda(tokens, out_len)
    if tokens.dtype != torch.int64 or tokens.shape[:-1] != out_len.shape:
        raise L.OtransHipError('%s: tokens int64 [..., T] and out_len [...] expected, got %s %s %s'
                               % (who, tokens.dtype, tuple(tokens.shape), tuple(out_len.shape)))
    T = tokens.shape[-1]
    tok, ln = tokens.contiguous(), out_len.to(torch.int32).contiguous()
    out = torch.empty(out_len.shape, dtype=torch.float32, device=tokens.device)
    return tok, ln, T, out


def ngram_score_sequences(ngram, tokens, out_len, alpha=1.0, beta=0.0, eos=1, with_logp=False):
    """Sentence scores of an NGramLM on the device (include/otrans_hip.h otr_ngram_score_seqs).  tokens int64 [..., T] (negative =
    padding), out_len int32 [...] lengths -> f32 [...] = alpha * (sum of ln P over the tokens and </s>) + beta * length; with_logp: also
    the bare sum.  One launch on the current stream, the same bits on every run, capturable."""
    tok, ln, T, out = _score_sequences_args('ngram_score_sequences', tokens, out_len)
    logp = torch.empty_like(out) if with_logp else None
    L.check(L.load().otr_ngram_score_seqs(*_ngram_args(ngram, out.device), _p(tok) if T else None, _p(ln), ln.numel(), T, float(alpha),
                                          float(beta), ngram.oov_score, int(eos), _p(out), _p(logp), _stream()), 'otr_ngram_score_seqs')
    return (out, logp) if with_logp else out


# ------------------------------------------------------------------ phrase biasing (csrc/bias.hip)
def _bias_args(bias, dev):
    """the table arguments both phrase-biasing entries take, in the order of include/otrans_hip.h"""
    return _p(bias.device_table(dev)), bias.capacity, bias.max_probe, bias.n_nodes, bias.max_len, bias.vocab_size


def bias_score_candidates(bias, preds, cand_idx, cand_score, eos, t=0, pos=None, flags=None, beam=0, cand_out=None, with_add=False,
                          k_score=None, k_idx=None):
    """The phrase-biasing addend of the pre-beam candidates (include/otrans_hip.h otr_bias_score_cands), the twin of
    ngram_score_candidates with a bias.PhraseBias in the n-gram's place: preds int64 [R, ldp] (row r's prefix is preds[r, :t], t = pos + 1
    with pos a device int32 scalar, when given; column 0 stands for BOS and is no token), cand_idx int32 / cand_score f32 [R, K'], flags
    u8 [R] marks finished rows (copied unchanged).  cand_out (default: a new tensor; may be cand_score itself) = cand_score +
    psi_minus(state(g c)) - psi(state(g)).  beam > 0: also the top-`beam` of each row in the prune's layout.  Returns (cand_out, cand_add
    or None, k_score, k_idx).  One launch on the current stream, no host synchronisation: capturable (call bias.to(device) before)."""
    return _score_candidates('bias_score_candidates', 'otr_bias_score_cands', _bias_args, bias, (), preds, cand_idx, cand_score, eos, t,
                             pos, flags, beam, cand_out, with_add, k_score, k_idx)


def bias_score_sequences(bias, tokens, out_len, eos=1):
    """The phrase-biasing score of whole hypotheses (include/otrans_hip.h otr_bias_score_seqs): tokens int64 [..., T] (negative =
    padding), out_len int32 [...] lengths -> f32 [...] = the summed addends of h + EOS: what the completed phrases of h earned.  One
    launch on the current stream, the same bits on every run, capturable."""
    tok, ln, T, out = _score_sequences_args('bias_score_sequences', tokens, out_len)
    L.check(L.load().otr_bias_score_seqs(*_bias_args(bias, out.device), _p(tok) if T else None, _p(ln), ln.numel(), T, int(eos), _p(out),
                                         _stream()), 'otr_bias_score_seqs')
    return out


CTC_ALIGN_MAX_TGT = 127


def _ctc_path_setup(who, ws_bytes, log_probs, in_len, targets, tgt_len, blank, ok=True, more=''):
    """what ctc_forced_align and ctc_segment share behind their own check of targets' width: the device, log_probs and "bad arguments"
    checks (ok, more: the caller's own condition and its part of that message), the operands as the library takes them, the workspace
    of ws_bytes(B, T, max_tgt) bytes and the four common outputs"""
    _cuda(log_probs, in_len, targets, tgt_len)
    if log_probs.dim() != 3 or log_probs.dtype != torch.float32:
        raise L.OtransHipError('%s: log_probs must be f32 [B, T, V], got %s %s' % (who, log_probs.dtype, tuple(log_probs.shape)))
    B, T, V = log_probs.shape
    max_tgt = targets.shape[1]
    dev = log_probs.device
    lp = log_probs if log_probs.stride(2) == 1 and log_probs.stride(0) == T * log_probs.stride(1) else log_probs.contiguous()
    tg = targets.to(torch.int64)
    if max_tgt == 0:                                  # no label column (ctc_forced_align only): the library still wants a row to point at
        tg = torch.zeros((B, 1), dtype=torch.int64, device=dev)
    elif tg.stride(1) != 1:
        tg = tg.contiguous()
    il = in_len.to(torch.int32).contiguous()
    tl = tgt_len.to(torch.int32).contiguous()
    need = getattr(L.load(), ws_bytes)(B, T, max_tgt)
    if need < 0 or not ok or targets.shape[0] != B or il.numel() != B or tl.numel() != B or not 0 <= blank < V:
        raise L.OtransHipError('%s: bad arguments B=%d T=%d V=%d targets %s blank=%d%s' % (who, B, T, V, tuple(targets.shape), blank, more))
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    frame_token = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, max_tgt, 2), dtype=torch.int32, device=dev)
    label_logp = torch.empty((B, max_tgt), dtype=torch.float32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    return lp, tg, il, tl, ws, need, (frame_token, spans, label_logp, score)


def ctc_forced_align(log_probs, in_len, targets, tgt_len, blank=0):
    """CTC forced alignment on the device (include/otrans_hip.h otr_ctc_align): the most probable CTC path of each utterance's known
    label sequence.  log_probs f32 [B, T, V] (log-softmax output), in_len [B] frames, targets int64 [B, max_tgt] labels, tgt_len [B]
    their counts.  Returns (frame_token int32 [B, T]: the path's token per frame, blank on blank frames, -1 past in_len; spans int32
    [B, max_tgt, 2]: first and one-past-last frame of each label, -1 past tgt_len; label_logp f32 [B, max_tgt]: the label's log-probs
    summed over its span; score f32 [B]: the path's log-probability).  An utterance that cannot be aligned (fewer frames than labels
    plus adjacent repeats, a length beyond max_tgt) has score -inf, frame_token and spans -1, label_logp 0.  No autograd; one launch
    on the current stream, no host synchronisation."""
    if targets.dim() != 2 or targets.shape[1] > CTC_ALIGN_MAX_TGT:
        raise ValueError('ctc_forced_align: targets must be [B, max_tgt] with max_tgt <= %d label columns, got %s'
                         % (CTC_ALIGN_MAX_TGT, tuple(targets.shape)))
    lp, tg, il, tl, ws, need, outs = _ctc_path_setup('ctc_forced_align', 'otr_ctc_align_workspace_bytes', log_probs, in_len, targets,
                                                     tgt_len, blank)
    (B, T, V), max_tgt = lp.shape, targets.shape[1]
    frame_token, spans, label_logp, score = outs
    lib = L.load()
    if max_tgt == 0:                                  # empty outputs have no address
        spans = label_logp = torch.empty(2, dtype=torch.int32, device=lp.device)
    L.check(_timed('ctc_align %dx%dx%d' % (B, T, max_tgt), {'bytes': B * T * (2 * max_tgt + 1) * 4},
                   lambda: lib.otr_ctc_align(_p(lp), lp.stride(1), _p(tg), tg.stride(0), _p(il), _p(tl), B, T, V, max_tgt, blank,
                                                  _p(ws), need, _p(frame_token), _p(spans), _p(label_logp), _p(score), _stream())),
            'otr_ctc_align')
    return outs


CTC_SEGMENT_MAX_TGT = 4095


def ctc_segment(log_probs, in_len, targets, tgt_len, blank=0, free_start=True, free_end=True, skip_logp=0.0):
    """CTC segmentation on the device (include/otrans_hip.h otr_ctc_segment): the most probable CTC path of each recording's known
    label sequence (up to 4095 labels) that may begin after the recording's first frame (free_start) and end before its last
    (free_end); every frame it leaves out is charged skip_logp <= 0.  Arguments as ops.ctc_forced_align.  Returns (frame_token int32
    [B, T]: the path's token per covered frame, blank on blank frames, -1 on skipped frames and past in_len; spans int32 [B, max_tgt,
    2]; label_logp f32 [B, max_tgt]; score f32 [B]; bounds int32 [B, 2]: the first covered frame and one past the last).  A
    recording that cannot be segmented (no labels, no frames, fewer frames than labels plus adjacent repeats, a length beyond
    max_tgt) has score -inf, frame_token, spans and bounds -1, label_logp 0.  With both flags off and at most 127 labels the first
    four outputs are ctc_forced_align's.  No autograd; one launch on the current stream, no host synchronisation."""
    if targets.dim() != 2 or not 1 <= targets.shape[1] <= CTC_SEGMENT_MAX_TGT:
        raise ValueError('ctc_segment: targets must be [B, max_tgt] with 1 <= max_tgt <= %d label columns, got %s'
                         % (CTC_SEGMENT_MAX_TGT, tuple(targets.shape)))
    skip_logp = float(skip_logp)
    lp, tg, il, tl, ws, need, outs = _ctc_path_setup('ctc_segment', 'otr_ctc_segment_workspace_bytes', log_probs, in_len, targets, tgt_len,
                                                     blank, math.isfinite(skip_logp) and skip_logp <= 0.0, ' skip_logp=%r' % skip_logp)
    (B, T, V), max_tgt = lp.shape, targets.shape[1]
    frame_token, spans, label_logp, score = outs
    bounds = torch.empty((B, 2), dtype=torch.int32, device=lp.device)
    lib = L.load()
    L.check(_timed('ctc_segment %dx%dx%d' % (B, T, max_tgt), {'bytes': B * T * (2 * max_tgt + 1) * 4},
                   lambda: lib.otr_ctc_segment(_p(lp), lp.stride(1), _p(tg), tg.stride(0), _p(il), _p(tl), B, T, V, max_tgt, blank,
                                                    int(bool(free_start)), int(bool(free_end)), skip_logp, _p(ws), need, _p(frame_token),
                                                    _p(spans), _p(label_logp), _p(score), _p(bounds), _stream())), 'otr_ctc_segment')
    return outs + (bounds,)


# ------------------------------------------------------------------ WER / CER scoring (csrc/editdist.hip)
EDIT_MAX_LEN, EDIT_MAX_NBEST = 2048, 32


def _rows_by_stride(t):
    """int64 tokens whose last dimension is contiguous: widened / copied only where needed, outer strides kept"""
    t = t.to(torch.int64)
    return t if t.shape[-1] <= 1 or t.stride(-1) == 1 else t.contiguous()


def _hyp_rows(hyp, hyp_len):
    """hypotheses int [B, N, L] and their lengths as the entries take them; hyp_len None: the full width"""
    B, N, Lh = hyp.shape
    return _rows_by_stride(hyp), (torch.full((B, N), Lh, dtype=torch.int32, device=hyp.device) if hyp_len is None
                                  else hyp_len.to(torch.int32).reshape(B, N).contiguous())


def _edit_pair_args(who, max_len, ref, ref_len, hyp, hyp_len):
    """the checks and the operands edit_distance and edit_align share, each with its own width limit -> (r, rl, h, hl, B, N, Lr, Lh)"""
    if hyp.dim() == 2:
        hyp = hyp.unsqueeze(1)
    if ref.dim() != 2 or hyp.dim() != 3 or hyp.shape[0] != ref.shape[0]:
        raise ValueError('%s: ref must be [B, Lr] and hyp [B, N, Lh] or [B, Lh], got %s and %s' % (who, tuple(ref.shape), tuple(hyp.shape)))
    B, N, Lh = hyp.shape
    Lr = ref.shape[1]
    if not 1 <= N <= EDIT_MAX_NBEST:
        raise ValueError('%s: %d hypotheses per utterance, 1 .. %d supported' % (who, N, EDIT_MAX_NBEST))
    if Lr > max_len or Lh > max_len:
        raise ValueError('%s: widths Lr=%d Lh=%d, at most %d supported' % (who, Lr, Lh, max_len))
    _cuda(ref, ref_len, hyp, hyp_len)
    if ref.dtype not in (torch.int32, torch.int64) or hyp.dtype not in (torch.int32, torch.int64):
        raise L.OtransHipError('%s: tokens must be int32 or int64, got %s and %s' % (who, ref.dtype, hyp.dtype))
    r, (h, hl) = _rows_by_stride(ref), _hyp_rows(hyp, hyp_len)
    rl = ref_len.to(torch.int32).contiguous()
    if rl.numel() != B or min(r.stride(0), h.stride(0), h.stride(1)) < 0:
        raise L.OtransHipError('%s: bad arguments ref %s ref_len %s hyp %s' % (who, tuple(ref.shape), tuple(ref_len.shape), tuple(hyp.shape)))
    return r, rl, h, hl, B, N, Lr, Lh


def edit_distance(ref, ref_len, hyp, hyp_len=None, eos=-1, totals=None):
    """Edit distance of n-best hypotheses against their references on the device (include/otrans_hip.h otr_edit_distance).  ref int
    [B, Lr] tokens, ref_len [B]; hyp int [B, N, Lh] (or [B, Lh]: N = 1, the outputs keep the N axis), hyp_len [B, N] (None: the full
    width, useful with eos); eos >= 0: a hypothesis ends before its first eos.  Pair (b, n) scores hypothesis n of utterance b against
    reference b.  Returns (dist int32 [B, N], counts int32 [B, N, 3] = substitutions / deletions / insertions of the canonical
    alignment, totals int64 [8] = {utterances, ref_tokens, errors_1best, S, D, I, errors_oracle, bad}); `totals` is accumulated into
    when given (a zeroed one is made otherwise).  A length outside its width gives -1s for the pair.  int32 tokens are widened; views
    with a contiguous last dimension are passed by stride.  One launch on the current stream, no host synchronisation, capturable."""
    r, rl, h, hl, B, N, Lr, Lh = _edit_pair_args('edit_distance', EDIT_MAX_LEN, ref, ref_len, hyp, hyp_len)
    dev = r.device
    if totals is None:
        totals = torch.zeros(8, dtype=torch.int64, device=dev)
    else:
        _cuda(totals)
        if totals.dtype != torch.int64 or totals.shape != (8,) or not totals.is_contiguous():
            raise L.OtransHipError('edit_distance: totals must be a contiguous int64 [8] tensor')
    dist = torch.empty((B, N), dtype=torch.int32, device=dev)
    counts = torch.empty((B, N, 3), dtype=torch.int32, device=dev)
    lib = L.load()
    L.check(_timed('edit_distance %dx%dx%dx%d' % (B, N, Lr, Lh), {'bytes': B * (Lr + N * Lh) * 8},
                   lambda: lib.otr_edit_distance(_p(r), r.stride(0), _p(rl), _p(h), h.stride(0), h.stride(1), _p(hl), B, N, Lr, Lh,
                                                 int(eos), _p(dist), _p(counts), _p(totals), _stream())), 'otr_edit_distance')
    return dist, counts, totals


# ------------------------------------------------------------------ per-token alignment, n-best consensus (csrc/nbest.hip)
NBEST_MAX_LEN = 256         # OTR_NBEST_MAX_LEN: the back-pointers of one pair stay in LDS


def edit_align(ref, ref_len, hyp, hyp_len=None, eos=-1):
    """The canonical alignment of ops.edit_distance, per hypothesis token (include/otrans_hip.h otr_edit_align).  The arguments, the eos
    cut and the validity rules are edit_distance's; widths up to NBEST_MAX_LEN.  Returns (dist int32 [B, N], code int8 [B, N, Lh]: 0
    match, 1 substitution, 2 insertion, -1 past the hypothesis's end, ref_pos int32 [B, N, Lh]: the reference token a match or a
    substitution is aligned to, -1 on insertions and past the end).  An invalid pair gives -1s.  int32 tokens are widened; views with a
    contiguous last dimension are passed by stride.  One launch on the current stream, no host synchronisation, capturable."""
    r, rl, h, hl, B, N, Lr, Lh = _edit_pair_args('edit_align', NBEST_MAX_LEN, ref, ref_len, hyp, hyp_len)
    dev = r.device
    dist = torch.empty((B, N), dtype=torch.int32, device=dev)
    code = torch.empty((B, N, Lh), dtype=torch.int8, device=dev)
    ref_pos = torch.empty((B, N, Lh), dtype=torch.int32, device=dev)
    lib = L.load()
    L.check(_timed('edit_align %dx%dx%dx%d' % (B, N, Lr, Lh), {'bytes': B * (Lr + N * Lh) * 8},
                   lambda: lib.otr_edit_align(_p(r), r.stride(0), _p(rl), _p(h), h.stride(0), h.stride(1), _p(hl), B, N, Lr, Lh,
                                              int(eos), _p(dist), _p(code), _p(ref_pos), _stream())), 'otr_edit_align')
    return dist, code, ref_pos


def nbest_consensus(tokens, lengths=None, scores=None, scale=1.0, eos=-1):
    """Consensus of an n-best on the device (include/otrans_hip.h otr_nbest_consensus): tokens int [B, N, L], lengths [B, N] (None: the
    full width, useful with eos), scores f32 [B, N] (None: all 0, a uniform posterior); eos >= 0: a hypothesis ends before its first
    eos.  A slot is live if its score is finite and its length fits the width.  Returns (post f32 [B, N]: softmax of scale * score over
    the live slots; risk f32 [B, N]: the expected edit distance of a hypothesis against the others under post, +inf on dead slots;
    best int32 [B]: the live slot of least risk, ties to the higher score, then the lower index, -1 where none is live; conf f32
    [B, N, L]: per token the posterior mass of the hypotheses whose alignment matches it, 0 past the end and on dead slots).  N up to
    EDIT_MAX_NBEST, L up to NBEST_MAX_LEN.  Two launches on the current stream, no host synchronisation, capturable; the sums run in
    a fixed order, so the outputs are the same bits on every run."""
    if tokens.dim() != 3:
        raise ValueError('nbest_consensus: tokens must be [B, N, L], got %s' % (tuple(tokens.shape),))
    B, N, Lh = tokens.shape
    if not 1 <= N <= EDIT_MAX_NBEST:
        raise ValueError('nbest_consensus: %d hypotheses per utterance, 1 .. %d supported' % (N, EDIT_MAX_NBEST))
    if Lh > NBEST_MAX_LEN:
        raise ValueError('nbest_consensus: width L=%d, at most %d supported' % (Lh, NBEST_MAX_LEN))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError('nbest_consensus: scale=%r must be finite' % (scale,))
    _cuda(tokens, lengths, scores)
    if tokens.dtype not in (torch.int32, torch.int64):
        raise L.OtransHipError('nbest_consensus: tokens must be int32 or int64, got %s' % (tokens.dtype,))
    dev = tokens.device
    h, hl = _hyp_rows(tokens, lengths)
    sc = (torch.zeros((B, N), dtype=torch.float32, device=dev) if scores is None
          else scores.to(torch.float32).reshape(B, N).contiguous())
    if min(h.stride(0), h.stride(1)) < 0:
        raise L.OtransHipError('nbest_consensus: bad arguments tokens %s' % (tuple(tokens.shape),))
    post = torch.empty((B, N), dtype=torch.float32, device=dev)
    risk = torch.empty((B, N), dtype=torch.float32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    conf = torch.empty((B, N, Lh), dtype=torch.float32, device=dev)
    lib = L.load()
    L.check(_timed('nbest_consensus %dx%dx%d' % (B, N, Lh), {'bytes': B * N * Lh * 12},
                   lambda: lib.otr_nbest_consensus(_p(h), h.stride(0), h.stride(1), _p(hl), _p(sc), scale, B, N, Lh, int(eos), _p(post),
                                                   _p(risk), _p(best), _p(conf), _stream())), 'otr_nbest_consensus')
    return post, risk, best, conf


# ------------------------------------------------------------------ joint CTC/attention beam search (csrc/ctcscore.hip)
JOINT_MAX_K, JOINT_MAX_T, JOINT_MAX_V, JOINT_MAX_BEAM = 32, 2048, 8192, 16


def joint_prebeam(logits, lm_logits, att_weight, lm_weight, k, V, cand_score=None, cand_idx=None):
    """The pre-beam of the joint search (include/otrans_hip.h otr_joint_prebeam): per row of logits f32 [R, >= V] (and lm_logits,
    or None) the k tokens of highest att_weight * log_softmax(logits) + lm_weight * log_softmax(lm_logits), descending, ties -> lower
    token.  Returns (cand_score f32 [R, k], cand_idx int32 [R, k]); one launch on the current stream, capturable."""
    _cuda(logits)
    R = logits.shape[0]
    dev = logits.device
    if cand_score is None:
        cand_score = torch.empty((R, k), dtype=torch.float32, device=dev)
        cand_idx = torch.empty((R, k), dtype=torch.int32, device=dev)
    L.check(L.load().otr_joint_prebeam(_p(logits), logits.stride(0), _p(lm_logits), lm_logits.stride(0) if lm_logits is not None else V,
                                       float(att_weight), float(lm_weight), R, V, k, _p(cand_score), _p(cand_idx), _stream()),
            'otr_joint_prebeam')
    return cand_score, cand_idx


def ctc_prefix_score(log_probs, lengths, cand_idx, preds, t, rows_per_utt, blank, eos, jsrc, state_in, state_out, pos=None,
                     cand_score=None, ctc_weight=0.0, beam=0, flags=None, k_score=None, k_idx=None, k_src=None):
    """CTC prefix scores of every candidate extension (include/otrans_hip.h otr_ctc_prefix_score).  log_probs f32 [B, T', V] (the CTC
    head's log-softmax), lengths int32 [B] frames; cand_idx int32 [R, K'] candidate tokens of the R hypotheses whose prefixes are
    preds[:, :t] (t = pos + 1 with pos a device int32 scalar, when given); jsrc int32 [R]: each hypothesis's slot in state_in.
    state_in / state_out: (rn f32 [slots, T'], rb f32 [slots, T'], psi f32 [slots]) -- state_out gets slot r*K'+k for every candidate
    (rn / rb may be None: psi only).  With cand_score f32 [R, K'] also the joint score and the top-`beam` of the K' per hypothesis into
    (k_score, k_idx, k_src).  One launch on the current stream, no host synchronisation: capturable."""
    _cuda(log_probs, lengths, cand_idx, preds)
    B, T, V = log_probs.shape
    R, K = cand_idx.shape
    rn_o, rb_o, psi_o = state_out
    L.check(L.load().otr_ctc_prefix_score(_p(log_probs), log_probs.stride(1), _p(lengths), B, T, V, blank, eos, R, rows_per_utt, K,
                                          _p(cand_idx), _p(cand_score), _p(flags), _p(preds), preds.stride(0), int(t), _p(pos), _p(jsrc),
                                          _p(state_in[0]), _p(state_in[1]), _p(state_in[2]), float(ctc_weight), _p(rn_o), _p(rb_o),
                                          _p(psi_o), int(beam), _p(k_score), _p(k_idx), _p(k_src), _stream()), 'otr_ctc_prefix_score')
    return psi_o


# ------------------------------------------------------------------ attention rescoring of the CTC n-best (csrc/rescore.hip)
RESCORE_MAX_W, RESCORE_MAX_V = 32, 8192


def _rescore_check(who, W, V, nbest, ctc_weight):
    """the limits of include/otrans_hip.h, refused on the host before the first launch"""
    if not 1 <= int(W) <= RESCORE_MAX_W:
        raise ValueError('%s: W=%d hypotheses per utterance must be in [1, %d]' % (who, W, RESCORE_MAX_W))
    if not 1 <= int(V) <= RESCORE_MAX_V:
        raise ValueError('%s: vocabulary V=%d must be in [1, %d]' % (who, V, RESCORE_MAX_V))
    if not 1 <= int(nbest) <= int(W):
        raise ValueError('%s: nbest=%d must be in [1, W=%d]' % (who, nbest, W))
    if not 0.0 <= float(ctc_weight) <= 1.0:
        raise ValueError('%s: ctc_weight=%r must be in [0, 1]' % (who, ctc_weight))


def rescore_pack(tokens, out_len, scores, max_len, V, bos=1, eos=1):
    """The CTC beam (ops.ctc_prefix_beam_search's tokens int64 [B, W, T] padded with -1, out_len [B, W], scores [B, W]) as ONE
    teacher-forced decoder batch (include/otrans_hip.h otr_rescore_pack): ys_in int64 [B*W, max_len] = BOS, the tokens, EOS filler;
    ys_out int64 [B*W, max_len] = the tokens, EOS, then -1; n_rows int32 [B*W] = len + 1, or 0 for a dead or too long slot.  One launch
    on the current stream, capturable."""
    B, W, T = tokens.shape
    _rescore_check('rescore_pack', W, V, 1, 0.0)
    _cuda(tokens, out_len, scores)
    if tokens.dtype != torch.int64 or out_len.dtype != torch.int32 or scores.dtype != torch.float32:
        raise L.OtransHipError('rescore_pack: tokens int64, out_len int32, scores f32 expected')
    tokens, out_len, scores = tokens.contiguous(), out_len.contiguous(), scores.contiguous()
    dev = tokens.device
    ys_in = torch.empty((B * W, max_len), dtype=torch.int64, device=dev)
    ys_out = torch.empty((B * W, max_len), dtype=torch.int64, device=dev)
    n_rows = torch.empty((B * W,), dtype=torch.int32, device=dev)
    L.check(L.load().otr_rescore_pack(_p(tokens), _p(out_len), _p(scores), B * W, T, int(max_len), int(V), int(bos), int(eos), _p(ys_in),
                                      _p(ys_out), _p(n_rows), _stream()), 'otr_rescore_pack')
    return ys_in, ys_out, n_rows


def attention_rescore(logits, tokens, out_len, scores, max_len, V, ctc_weight, lm_logits=None, lm_weight=0.0, nbest=1, penalty=0.0,
                      lamda=5.0, packed=None, bos=1, eos=1, add_score=None):
    """The second pass of two-pass decoding after the decoder (include/otrans_hip.h otr_rescore_*).  logits f32 [B*W * max_len, >= V]
    (any leading shape; unit stride along the vocabulary): the teacher-forced decoder output on rescore_pack's ys_in; lm_logits the same
    from the language model, or None.  tokens / out_len / scores: the search's outputs.  total = (1 - ctc_weight) att + ctc_weight ctc
    + lm_weight lm (/ the length penalty), sorted descending, ties to the lower CTC rank, dead and too long slots (-inf) last.
    `packed`: rescore_pack's result for these hypotheses (else it is formed here: one more launch).
    `add_score`: f32 [B, W] in CTC order, added to total before the penalty's division (otr_rescore_select_add; the n-gram term).
    Returns a dict: tokens int64 [B, nbest, T] (-1 padded), len int32 [B, nbest], scores f32 [B, nbest], perm int32 [B, W] (rank -> CTC
    slot), total / att / lm f32 [B, W] in CTC order (lm None without lm_logits).  Two launches, no host synchronisation: capturable."""
    B, W, T = tokens.shape
    _rescore_check('attention_rescore', W, V, nbest, ctc_weight)
    _cuda(logits, tokens, out_len, scores)
    nh = B * W

    def rows(t, who):
        if t.dtype != torch.float32 or t.stride(-1) != 1 or t.shape[-1] < V:
            raise L.OtransHipError('attention_rescore: %s must be f32 with >= V=%d contiguous columns' % (who, V))
        t2 = t.reshape(-1, t.shape[-1])
        if t2.shape[0] != nh * max_len:
            raise L.OtransHipError('attention_rescore: %s has %d rows, B*W*max_len = %d expected' % (who, t2.shape[0], nh * max_len))
        return t2 if t2.stride(1) == 1 and t2.stride(0) >= V else t2.contiguous()
    lg = rows(logits, 'logits')
    lmg = rows(lm_logits, 'lm_logits') if lm_logits is not None else None
    tokens, out_len, scores = tokens.contiguous(), out_len.contiguous(), scores.contiguous()
    _, ys_out, n_rows = packed if packed is not None else rescore_pack(tokens, out_len, scores, max_len, V, bos, eos)
    dev = tokens.device
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)    # noqa: E731
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)      # noqa: E731
    att, lm = f32(B, W), (f32(B, W) if lmg is not None else None)
    total, perm = f32(B, W), i32(B, W)
    nb_tok, nb_len, nb_score = torch.empty((B, nbest, T), dtype=torch.int64, device=dev), i32(B, nbest), f32(B, nbest)
    lib = L.load()
    L.check(lib.otr_rescore_score(_p(lg), lg.stride(0), _p(lmg), lmg.stride(0) if lmg is not None else 0, _p(ys_out), ys_out.stride(0),
                                  _p(n_rows), nh, int(max_len), int(V), _p(att), _p(lm), _stream()), 'otr_rescore_score')
    sel = (_p(tokens), _p(out_len), _p(scores), _p(n_rows), _p(att), _p(lm))
    tail = (B, W, T, int(nbest), float(ctc_weight), float(lm_weight or 0.0), float(penalty or 0.0), float(lamda), _p(total), _p(perm),
            _p(nb_tok), _p(nb_len), _p(nb_score), _stream())
    if add_score is None:
        L.check(lib.otr_rescore_select(*sel, *tail), 'otr_rescore_select')
    else:
        _cuda(add_score)
        if add_score.dtype != torch.float32 or add_score.numel() != nh:
            raise L.OtransHipError('attention_rescore: add_score must be f32 [B, W], got %s %s' % (add_score.dtype, tuple(add_score.shape)))
        L.check(lib.otr_rescore_select_add(*sel, _p(add_score.contiguous()), *tail), 'otr_rescore_select_add')
    return {'tokens': nb_tok, 'len': nb_len, 'scores': nb_score, 'perm': perm, 'total': total, 'att': att, 'lm': lm}
