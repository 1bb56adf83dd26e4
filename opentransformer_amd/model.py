"""Model assembly: SpeechToText (otrans/model/speech2text.py:15-90) and the CTC head
(otrans/model/ctc.py:12-66) built from the drop-in registries of this package."""
import contextlib
import dataclasses

import torch
import torch.nn as nn

from . import ops
from .nn import (BLK, EOS, ConformerEncoder, ConvFrontEnd, LabelSmoothingLoss, TransformerDecoder, TransformerEncoder,
                 _unsupported)

BuildFrontEnd = {'conv': ConvFrontEnd}                 # otrans/frontend/__init__.py:8-12
BuildEncoder = {'transformer': TransformerEncoder, 'conformer': ConformerEncoder}     # otrans/encoder/__init__.py:10-13
BuildDecoder = {'transformer': TransformerDecoder}     # otrans/decoder/__init__.py:8-10


def shift_targets(truth, stacked=False):
    """(decoder input, loss target) of a target matrix [B, L + 1]: truth[:, :-1] and truth[:, 1:] (speech2text.py:53,57 clones each).
    The embedding and the loss kernels read the two shifted VIEWS in place (row stride L + 1, no launch) when the matrix is on the
    device with unit inner stride; otherwise, or with `stacked` (a CTC term wants its targets contiguous), one launch copies both."""
    if stacked or not truth.is_cuda or truth.stride(-1) != 1:
        shifted = torch.stack((truth[:, :-1], truth[:, 1:]))
        return shifted[0], shifted[1]
    return truth[:, :-1], truth[:, 1:]


@contextlib.contextmanager
def evaluating(module):
    """`module` in eval() for the duration; every sub-module's `training` flag is put back afterwards, also after an exception"""
    modes = [(m, m.training) for m in module.modules()]
    module.eval()
    try:
        yield module
    finally:
        for m, was in modes:
            m.training = was


@dataclasses.dataclass
class TeacherForced:
    """What one teacher-forced pass of a model computed; a field is None where its head took no part (a CTCModel has no decoder)."""
    loss: torch.Tensor                   # the model's own loss: ce, ctc or (1 - ctc_weight) * ce + ctc_weight * ctc
    logits: torch.Tensor = None          # decoder logits [B, L, V], their loss target [B, L] and their cross-entropy
    target_out: torch.Tensor = None
    ce: torch.Tensor = None
    ctc_logits: torch.Tensor = None      # the CTC head's logits [B, T', V], the frames per utterance [B] and the CTC loss
    memory_length: torch.Tensor = None
    ctc: torch.Tensor = None


class AcousticModel(nn.Module):
    """frontend -> encoder, the first half of every pass of SpeechToText and CTCModel"""

    def encode(self, inputs, inputs_mask, mark=False):
        """(memory, memory_mask).  mark: everything behind this point finishes its backward before the encoder's starts (dp.py)"""
        enc_inputs, enc_mask = self.frontend(inputs, inputs_mask)
        memory, memory_mask, _ = self.encoder(enc_inputs, enc_mask)
        return (ops.early_mark(memory, self) if mark else memory), memory_mask

    def set_epoch(self, epoch):
        pass


class ModelTraining(nn.Module):
    """A training objective around the submodule `model` (FusedAdam / FlatDataParallel see the same parameters under `model.`)."""

    def save_checkpoint(self, params, name):
        return self.model.save_checkpoint(params, name)

    def load_model(self, chkpt):
        return self.model.load_model(chkpt)

    def set_epoch(self, epoch):
        return self.model.set_epoch(epoch)

    def scale_loss_grad(self, loss):
        """ops.scale_loss_grad with the loss scale the optimizer registered on this wrapper or, failing that, on the model"""
        return ops.scale_loss_grad(loss, self if getattr(self, '_otr_loss_scale', None) is not None else self.model)


class CTCAssistor(nn.Module):
    """model/ctc.py:12-66: Linear(d -> V) + log_softmax + CTC loss (blank 0, zero_infinity, 'mean')."""

    def __init__(self, hidden_size, vocab_size, blank=BLK, lookahead_steps=-1):
        super().__init__()
        self.lookahead_steps, self.apply_look_ahead, self.blank = lookahead_steps, lookahead_steps > 0, blank
        if self.apply_look_ahead:
            if lookahead_steps > 6 or hidden_size % 4:
                _unsupported('CTCAssistor lookahead_steps > 6 (the depthwise-conv kernels hold at most 7 taps)')
            self.lookahead_conv = nn.Conv1d(hidden_size, hidden_size, lookahead_steps + 1, padding=0, stride=1, bias=False,
                                            groups=hidden_size)         # parameter container only (model/ctc.py:17-24)
        self.output_layer = nn.Linear(hidden_size, vocab_size)

    def _look_ahead(self, memory):
        return ops.LookaheadConvFn.apply(memory, self.lookahead_conv.weight) if self.apply_look_ahead else memory

    def compute_logits(self, enc_states):
        return ops.linear(enc_states, self.output_layer.weight, self.output_layer.bias)

    def forward(self, memory, memory_length=None, targets=None, tgt_length=None, return_logits=False):
        logits = self.compute_logits(self._look_ahead(memory))
        if return_logits:
            return logits
        return self.compute_loss(logits, memory_length, targets, tgt_length)

    def compute_loss(self, logits, enc_length, targets, targets_length):
        return ops.CTCLossFn.apply(logits, targets, enc_length, targets_length, self.blank)

    def inference(self, memory, memory_mask):
        logits = self.compute_logits(self._look_ahead(memory))
        memory_length = torch.sum(memory_mask.squeeze(1) if memory_mask.dim() == 3 else memory_mask, dim=-1)
        return ops.log_softmax(logits), memory_length

    @torch.no_grad()
    def align(self, memory, memory_mask, labels, labels_length):
        """CTC forced alignment of `labels` [B, max_tgt] (plain units, `labels_length` [B] of them) on this head's log-probs:
        (frame_token, spans, label_logp, score) of ops.ctc_forced_align, in encoder frames"""
        log_probs, memory_length = self.inference(memory, memory_mask)
        return ops.ctc_forced_align(log_probs, memory_length, labels, labels_length, blank=self.blank)


class SpeechToText(AcousticModel):
    """model/speech2text.py:15-90.  forward(inputs: dict, targets: dict) -> (loss, aux | None)."""

    def __init__(self, params):
        super().__init__()
        self.frontend = BuildFrontEnd[params['frontend_type']](**params['frontend'])
        self.encoder = BuildEncoder[params['encoder_type']](**params['encoder'])
        self.decoder = BuildDecoder[params['decoder_type']](**params['decoder'])
        self.crit = LabelSmoothingLoss(size=params['decoder']['vocab_size'], smoothing=params['smoothing'])
        self.ctc_weight = params['ctc_weight']
        if self.ctc_weight > 0.0:
            self.assistor = CTCAssistor(hidden_size=params['encoder_output_size'],
                                        vocab_size=params['decoder']['vocab_size'],
                                        lookahead_steps=params['lookahead_steps'] if 'lookahead_steps' in params else 0)

    def teacher_forced(self, memory, memory_mask, targets, ctc=None, grad_scale=None):
        """The decoder on the shifted targets, its cross-entropy and, with `ctc` (default: the model has a CTC term), the head's CTC
        loss on the same targets (the EOS kept) and the model's mix of the two.  grad_scale: see LabelSmoothingLoss.root."""
        truth, truth_length = targets['targets'], targets['targets_length']
        ctc = self.ctc_weight > 0 if ctc is None else ctc
        dec_in, target_out = shift_targets(truth, stacked=ctc)
        logits, _ = self.decoder(dec_in, memory, memory_mask)
        ce = self.crit(logits, target_out) if grad_scale is None else self.crit.root(logits, target_out, grad_scale)
        out = TeacherForced(loss=ce, logits=logits, target_out=target_out, ce=ce)
        if ctc:
            out.memory_length = torch.sum(memory_mask, dim=-1)
            out.ctc_logits = self.assistor(memory, return_logits=True)
            out.ctc = self.assistor.compute_loss(out.ctc_logits, out.memory_length, target_out, truth_length)
            out.loss = (1 - self.ctc_weight) * ce + self.ctc_weight * out.ctc
        return out

    def forward(self, inputs, targets):
        memory, memory_mask = self.encode(inputs['inputs'], inputs['mask'], mark=True)
        if self.ctc_weight <= 0 and isinstance(self.crit, LabelSmoothingLoss):
            # the loss is the root of the backward pass: the factor it is seeded with (fp16 loss scale, ops.scale_loss_grad) rides in
            # the loss launch's gradient instead of two scalar-multiply launches
            return self.teacher_forced(memory, memory_mask, targets, grad_scale=ops.loss_scale_of(self)).loss, None
        out = self.teacher_forced(memory, memory_mask, targets)
        # the reference returns {'CTCLoss': loss_ctc.item()} (a host sync per step); we keep the tensor
        # scale_loss_grad: identity unless a loss scale is registered (fp16 training)
        return ops.scale_loss_grad(out.loss, self), {'CTCLoss': out.ctc.detach()} if out.ctc is not None else None

    def compute_ctc_loss(self, memory, memory_mask, targets_out, targets_length):
        memory_length = torch.sum(memory_mask, dim=-1)
        return self.assistor(memory, memory_length, targets_out, targets_length)

    @torch.no_grad()
    def align(self, inputs, inputs_mask, labels, labels_length):
        """CTC forced alignment with the model's CTC head.  `labels` [B, max_tgt] are plain units without BOS / EOS, `labels_length` [B]
        their counts.  The CTC term of forward() is trained on the labels followed by EOS (target_out = truth[:, 1:]), so that is the
        sequence aligned: frame_token [B, T'] (the EOS frames included) and score [B] are those of the whole path, spans
        [B, max_tgt, 2] and label_logp [B, max_tgt] are the labels' alone, the EOS column dropped."""
        if getattr(self, 'assistor', None) is None:
            raise ValueError('align needs the model\'s CTC head (model.assistor): build the model with ctc_weight > 0')
        n = labels_length.to(torch.int64)
        ext = torch.cat((labels.to(torch.int64), labels.new_zeros((labels.size(0), 1), dtype=torch.int64)), dim=1)
        ext.scatter_(1, n.clamp(0, labels.size(1)).unsqueeze(1), EOS)          # a length outside [0, max_tgt] stays infeasible below
        memory, memory_mask = self.encode(inputs, inputs_mask)
        frame_token, spans, label_logp, score = self.assistor.align(memory, memory_mask, ext, torch.where(n < 0, n, n + 1))
        keep = torch.arange(labels.size(1), device=labels.device).unsqueeze(0) < n.unsqueeze(1)       # the EOS is label n of its row
        spans = torch.where(keep.unsqueeze(-1), spans[:, :-1], torch.full_like(spans[:, :-1], -1))
        label_logp = torch.where(keep, label_logp[:, :-1], torch.zeros_like(label_logp[:, :-1]))
        return frame_token, spans, label_logp, score

    def save_checkpoint(self, params, name):
        checkpoint = {'params': params, 'frontend': self.frontend.state_dict(), 'encoder': self.encoder.state_dict(),
                      'decoder': self.decoder.state_dict()}
        if self.ctc_weight > 0.0:
            checkpoint['ctc'] = self.assistor.state_dict()
        torch.save(checkpoint, name)

    def load_model(self, chkpt):
        self.frontend.load_state_dict(chkpt['frontend'])
        self.encoder.load_state_dict(chkpt['encoder'])
        self.decoder.load_state_dict(chkpt['decoder'])
        if 'ctc' in chkpt and self.ctc_weight > 0.0:
            self.assistor.load_state_dict(chkpt['ctc'])


class CTCModel(AcousticModel):
    """model/ctc.py:69-140: frontend + encoder + CTC head.  forward(inputs, targets) -> (loss, None) with the labels
    truth[:, 1:-1] and lengths targets_length - 1 (:95; SpeechToText's joint CTC term keeps the EOS instead).  The
    reference's inference / recognize / ts_forward call the encoder without the frontend and with a length where a mask
    belongs (:98-121, broken as shipped); inference() here is the working form: frontend -> encoder ->
    CTCAssistor.inference, which is what recognize.CTCRecognizer consumes.  ts_forward (:105-115, the teacher-student forward: the
    head's raw logits) has its working form in distill.DistillTraining, which reads teacher_forced(...).ctc_logits."""

    def __init__(self, params):
        super().__init__()
        self.frontend = BuildFrontEnd[params['frontend_type']](**params['frontend'])
        self.encoder = BuildEncoder[params['encoder_type']](**params['encoder'])
        self.assistor = CTCAssistor(hidden_size=params['encoder_output_size'], vocab_size=params['vocab_size'],
                                    lookahead_steps=params['lookahead_steps'] if 'lookahead_steps' in params else -1)

    def teacher_forced(self, memory, memory_mask, targets):
        """the head's logits and its CTC loss on the labels truth[:, 1:-1], which is the model's own loss"""
        truth, truth_length = targets['targets'], targets['targets_length']
        memory_length = torch.sum(memory_mask, dim=-1)
        labels, labels_length = truth[:, 1:-1].contiguous(), truth_length.add(-1)
        ctc_logits = self.assistor(memory, return_logits=True)
        ctc = self.assistor.compute_loss(ctc_logits, memory_length, labels, labels_length)
        return TeacherForced(loss=ctc, ctc_logits=ctc_logits, memory_length=memory_length, ctc=ctc)

    def forward(self, inputs, targets):
        memory, memory_mask = self.encode(inputs['inputs'], inputs['mask'])
        return ops.scale_loss_grad(self.teacher_forced(memory, memory_mask, targets).loss, self), None

    def inference(self, inputs, inputs_mask):
        memory, memory_mask = self.encode(inputs, inputs_mask)
        return self.assistor.inference(memory, memory_mask)

    recognize = inference

    @torch.no_grad()
    def align(self, inputs, inputs_mask, labels, labels_length):
        """CTC forced alignment of `labels` [B, max_tgt] (plain units without BOS / EOS, `labels_length` [B] of them): the head is
        trained on the labels as they are (forward()), so they are aligned as they are.  Returns ops.ctc_forced_align's
        (frame_token, spans, label_logp, score) in encoder frames."""
        memory, memory_mask = self.encode(inputs, inputs_mask)
        return self.assistor.align(memory, memory_mask, labels, labels_length)

    def save_checkpoint(self, params, name):
        torch.save({'params': params, 'frontend': self.frontend.state_dict(), 'encoder': self.encoder.state_dict(),
                    'ctc': self.assistor.state_dict()}, name)

    def load_model(self, chkpt):
        self.frontend.load_state_dict(chkpt['frontend'])
        self.encoder.load_state_dict(chkpt['encoder'])
        self.assistor.load_state_dict(chkpt['ctc'])


End2EndModel = {'ctc': CTCModel, 'speech2text': SpeechToText}           # otrans/model/__init__.py:6-9
