"""Minimum word error rate (MWER) training of a SpeechToText model on the device: the beam search's n-best, the edit distance of
every hypothesis, one teacher-forced decoder pass over all of them and the N-best expected number of errors (Prabhavalkar et al. 2018;
include/otrans_hip.h otr_mwer_loss) with its gradient -- no copy to the host anywhere in the step.  CTCMWERTraining is the same objective for a CTCModel: the n-best of the
CTC prefix beam search, their edit distances, and the expected number of errors under the CTC likelihoods of the hypotheses, scored
on one log-softmax of the head's logits together with the CTC loss on the reference (include/otrans_hip.h otr_ctc_mwer_loss)."""
import torch

from . import ops
from .model import CTCModel, ModelTraining, evaluating
from .nn import BOS, EOS
from .recognize import CTCRecognizer, SpeechToTextRecognizer


class MWERTraining(ModelTraining):
    """Wraps a SpeechToText as the submodule `model` (FusedAdam / FlatDataParallel see the same parameters under `model.`);
    forward(inputs, targets, hyps=None) -> (loss, aux) with loss = MWER + ce_weight * the model's own cross-entropy.

    nbest hypotheses per utterance come from `recognizer` (default: SpeechToTextRecognizer(model, beam_width=beam_width or nbest,
    nbest=nbest, max_len=max_len, **search_kw), so lm / joint_ctc / ngram_lm ... shape the n-best), searched under no_grad with the
    model in eval() and the previous modes restored afterwards; or pass hyps = (tokens int64 [B, N, L], lengths int32 [B, N]).
    A hypothesis longer than max_len - 1 tokens takes no part (as in attention rescoring); N <= ops.MWER_MAX_NBEST.
    The training search defaults to the re-forward loop (apply_cache=False): the cached loop's captured graphs are keyed by the
    weights' version and would be rebuilt after every optimizer step (tools/mwer_bench.py measures both).
    aux: 'MWER', 'CE' (scalars), 'errors_1best', 'errors_oracle' (int32 [B]; -1: no valid hypothesis), 'post' (f32 [B, N], the
    posterior over the live hypotheses) -- device tensors, no host synchronisation."""

    def __init__(self, model, nbest=4, beam_width=None, max_len=50, ce_weight=0.01, recognizer=None, **search_kw):
        super().__init__()
        if isinstance(model, CTCModel):
            raise TypeError('MWERTraining trains a SpeechToText; a CTCModel has no decoder to teacher-force: use CTCMWERTraining')
        if not 1 <= int(nbest) <= ops.MWER_MAX_NBEST:
            raise ValueError('MWERTraining: nbest=%d must be in [1, %d]' % (nbest, ops.MWER_MAX_NBEST))
        if max_len < 1 or ce_weight < 0:
            raise ValueError('MWERTraining: max_len=%r must be >= 1 and ce_weight=%r >= 0' % (max_len, ce_weight))
        self.model = model
        self.nbest, self.max_len, self.ce_weight = int(nbest), int(max_len), float(ce_weight)
        if recognizer is None:
            search_kw.setdefault('apply_cache', False)
            with evaluating(model):                       # the recognizer's constructor puts the model into eval()
                recognizer = SpeechToTextRecognizer(model, beam_width=beam_width or nbest, nbest=nbest, max_len=max_len, **search_kw)
        self.recognizer = recognizer

    def search(self, inputs, inputs_mask):
        """the recognizer's n-best (tokens int64 [B, N, L], lengths int32 [B, N]) with the model in eval() for the duration"""
        with evaluating(self.model), torch.no_grad():
            tokens, lengths, _ = self.recognizer.recognize_tokens(inputs, inputs_mask)
        return tokens, lengths

    def forward(self, inputs, targets, hyps=None):
        model = self.model
        enc_inputs, enc_mask = inputs['inputs'], inputs['mask']
        truth, truth_length = targets['targets'], targets['targets_length']
        tokens, lengths = self.search(enc_inputs, enc_mask) if hyps is None else hyps
        B, N, L = tokens.shape
        if not 1 <= N <= ops.MWER_MAX_NBEST:
            raise ValueError('MWERTraining: %d hypotheses per utterance, 1 .. %d supported' % (N, ops.MWER_MAX_NBEST))
        tokens, lengths = tokens.to(torch.int64).contiguous(), lengths.to(torch.int32).reshape(B, N).contiguous()
        errors = ops.edit_distance(truth[:, 1:], truth_length - 1, tokens, lengths)[0]
        # one teacher-forced batch of all B x N hypotheses.  otr_rescore_pack reads tokens [0, length) of a slot only (a length
        # outside [0, L] makes the slot dead), so what lies behind a hypothesis needs no masking; rows past L + 1 could never be live
        V = model.decoder.output_layer.weight.shape[0]
        rows = min(self.max_len, L + 1)
        ys_in, ys_out, n_rows = ops.rescore_pack(tokens, lengths, torch.zeros((B, N), dtype=torch.float32, device=tokens.device), rows,
                                                 V, BOS, EOS)
        memory, memory_mask = model.encode(enc_inputs, enc_mask, mark=True)
        hidden = model.decoder.hidden(ys_in, memory, memory_mask, share=N)
        logits = ops.linear(hidden, model.decoder.output_layer.weight, model.decoder.output_layer.bias)
        mwer, stats = ops.mwer_loss(logits, ys_out, n_rows, errors)
        total, ce = mwer, None
        if self.ce_weight > 0:
            ce = model.teacher_forced(memory, memory_mask, targets, ctc=False).ce     # no CTC term: the targets are read in place
            total = mwer + self.ce_weight * ce
        valid = errors >= 0
        oracle = torch.where(valid, errors, torch.full_like(errors, torch.iinfo(torch.int32).max)).min(dim=1).values
        aux = {'MWER': mwer.detach(), 'CE': ce.detach() if ce is not None else torch.zeros_like(mwer.detach()),
               'errors_1best': errors[:, 0], 'errors_oracle': torch.where(valid.any(dim=1), oracle, torch.full_like(oracle, -1)),
               'post': stats['post']}
        return self.scale_loss_grad(total), aux


class CTCMWERTraining(ModelTraining):
    """MWER (sequence-discriminative) training of a CTCModel, wrapped as the submodule `model`; forward(inputs, targets, hyps=None) ->
    (loss, aux) with loss = MWER + ctc_weight * the model's own CTC loss, both from ONE log-softmax of the head's logits and one
    gradient (ops.ctc_mwer_loss; include/otrans_hip.h otr_ctc_mwer_loss).

    nbest hypotheses per utterance come from the CTC prefix beam search of `recognizer` (default: CTCRecognizer(model, mode='beam',
    beam_width=beam_width or nbest, **search_kw), so ngram_lm / bias / cutoff_top_n shape the n-best) on the model's own
    assistor.inference, searched under no_grad with the model in eval() and the previous modes restored afterwards; the search's
    own order is kept (mbr re-ordering is not applied) and its beam is cut to nbest.  Or pass hyps = (tokens int64 [B, N, L],
    lengths int32 [B, N]).  Slots past the live beam get errors = -1 and take no part, as does a hypothesis of more than 127 labels;
    the reference is what CTCModel.teacher_forced trains on, truth[:, 1:-1] with targets_length - 1 labels.  N <= ops.MWER_MAX_NBEST.
    P_n = softmax_n(scale * log p(hyp_n | x)).
    aux: 'MWER', 'CTC' (scalars), 'errors_1best', 'errors_oracle' (int32 [B]; -1: no valid hypothesis), 'post' (f32 [B, N], the
    posterior over the live hypotheses) -- device tensors, no host synchronisation."""

    def __init__(self, model, nbest=4, beam_width=None, ctc_weight=0.01, scale=1.0, recognizer=None, **search_kw):
        super().__init__()
        if not isinstance(model, CTCModel):
            raise TypeError('CTCMWERTraining trains a CTCModel, not a %s (MWERTraining is the one for a SpeechToText)' % type(model).__name__)
        if not 1 <= int(nbest) <= ops.MWER_MAX_NBEST:
            raise ValueError('CTCMWERTraining: nbest=%d must be in [1, %d]' % (nbest, ops.MWER_MAX_NBEST))
        if beam_width is not None and int(beam_width) < int(nbest):
            raise ValueError('CTCMWERTraining: beam_width=%d below nbest=%d' % (beam_width, nbest))
        if not 0 <= float(ctc_weight) < float('inf') or not 0 < float(scale) < float('inf'):
            raise ValueError('CTCMWERTraining: ctc_weight=%r must be finite and >= 0, scale=%r finite and > 0' % (ctc_weight, scale))
        self.model = model
        self.nbest, self.ctc_weight, self.scale = int(nbest), float(ctc_weight), float(scale)
        if recognizer is None:
            with evaluating(model):                       # the recognizer's constructor puts the model into eval()
                recognizer = CTCRecognizer(model, mode='beam', beam_width=int(beam_width or nbest), **search_kw)
        self.recognizer = recognizer

    def search(self, inputs, inputs_mask):
        """the beam search's n-best (tokens int64 [B, N, L] padded with -1, lengths int32 [B, N], dead bool [B, N]: slots past the live
        beam) with the model in eval() for the duration"""
        rec = self.recognizer
        with evaluating(self.model), torch.no_grad():
            log_probs, length = self.model.assistor.inference(*rec._encode(inputs, inputs_mask))
            tokens, lengths, scores = rec._beam_search(log_probs, length)
        n = self.nbest
        return tokens[:, :n], lengths[:, :n], scores[:, :n] == float('-inf')

    def forward(self, inputs, targets, hyps=None):
        model = self.model
        enc_inputs, enc_mask = inputs['inputs'], inputs['mask']
        truth, truth_length = targets['targets'], targets['targets_length']
        dead = None
        if hyps is None:
            tokens, lengths, dead = self.search(enc_inputs, enc_mask)
        else:
            tokens, lengths = hyps
        if tokens.dim() != 3 or lengths.numel() != tokens.shape[0] * tokens.shape[1]:
            raise ValueError('CTCMWERTraining: hyps must be (tokens [B, N, L], lengths [B, N]), got %s and %s'
                             % (tuple(tokens.shape), tuple(lengths.shape)))
        B, N, _ = tokens.shape
        if not 1 <= N <= ops.MWER_MAX_NBEST:
            raise ValueError('CTCMWERTraining: %d hypotheses per utterance, 1 .. %d supported' % (N, ops.MWER_MAX_NBEST))
        tokens, lengths = tokens.to(torch.int64), lengths.to(torch.int32).reshape(B, N)
        labels, labels_length = truth[:, 1:-1], truth_length - 1          # what CTCModel.teacher_forced trains on
        errors = ops.edit_distance(labels, labels_length, tokens, lengths)[0]
        if dead is not None:
            errors = errors.masked_fill(dead, -1)
        memory, memory_mask = model.encode(enc_inputs, enc_mask)
        logits = model.assistor(memory, return_logits=True)
        total, stats = ops.ctc_mwer_loss(logits, torch.sum(memory_mask, dim=-1), tokens, lengths, errors, ref=labels, ref_len=labels_length,
                                         ctc_weight=self.ctc_weight, scale=self.scale, blank=model.assistor.blank)
        valid = stats['seq_logp'] > float('-inf')                          # the live slots: what the loss counted
        oracle = torch.where(valid, errors, torch.full_like(errors, torch.iinfo(torch.int32).max)).min(dim=1).values
        aux = {'MWER': stats['mwer'], 'CTC': stats['ctc'], 'errors_1best': errors[:, 0],
               'errors_oracle': torch.where(valid.any(dim=1), oracle, torch.full_like(oracle, -1)), 'post': stats['post']}
        return self.scale_loss_grad(total), aux
