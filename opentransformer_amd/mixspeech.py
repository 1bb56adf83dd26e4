"""MixSpeech training on the device (Meng et al. 2021; the reference's Trainer(mixspeech=True), otrans/train/trainer.py:155-201):
utterances 2p and 2p + 1 of a batch are mixed frame by frame with one weight lam ~ Beta(alpha, alpha) per batch, the mixed half batch
keeps the mask and length of the longer utterance, and the loss is lam * loss(mixed, targets of 2p) + (1 - lam) * loss(mixed, targets
of 2p + 1).  The reference runs the whole model once per target set on the same mixed input; here the encoder runs ONCE and both
target sets are scored on its one memory -- the same function with dropout off, one draw of the dropout masks instead of two with it
on.  The mix is one launch (include/otrans_hip.h otr_mixspeech_mix) and the CTC term one call for both label sets (otr_ctc_loss_pair)."""
import numpy as np
import torch

from . import ops
from .model import CTCModel, ModelTraining, SpeechToText


class MixSpeechTraining(ModelTraining):
    """Wraps the model as the submodule `model` (FusedAdam / FlatDataParallel see the same parameters under `model.`);
    forward(inputs, targets, lam=None) -> (loss, aux).

    lam=None draws np.random.beta(alpha, alpha, size=(1)) from numpy's global generator, the reference's own call: a seeded run draws
    what the reference draws.  The float32 value goes into a persistent one-element device buffer (`lam_buffer`) with a non-blocking
    copy; a float writes that value; a one-element f32 device tensor is used as it is (a captured step reads it on every replay).
    Nothing in forward reads lam back to the host.

    With B utterances P = B // 2 pairs are formed; an odd last utterance takes no part (trainer.py:158-159).  A SpeechToText runs its
    decoder and label-smoothing loss once per target set on the one memory, ce = lam * ce_1 + (1 - lam) * ce_2, and with a CTC head
    ctc = ops.ctc_loss_pair on the head's logits (labels truth[:, 1:], the EOS kept, as in teacher_forced):
    loss = (1 - ctc_weight) * ce + ctc_weight * ctc = lam * loss_1 + (1 - lam) * loss_2.  A CTCModel: loss = ops.ctc_loss_pair with
    the labels truth[:, 1:-1] and lengths targets_length - 1.  The target sets are the even and odd rows of the target matrix, read
    in place as strided views.

    aux: 'Lambda', 'Loss_1', 'Loss_2', and 'CTCLoss' where there is a CTC head -- detached device scalars, no host synchronisation.
    In eval() nothing is mixed: forward returns self.model(inputs, targets) (trainer.py:259-268)."""

    def __init__(self, model, alpha=0.5):
        super().__init__()
        if not isinstance(model, (SpeechToText, CTCModel)):
            raise ValueError('MixSpeechTraining: the model must be a SpeechToText or a CTCModel, got %s' % type(model).__name__)
        if not (float(alpha) > 0.0 and float(alpha) != float('inf')):
            raise ValueError('MixSpeechTraining: alpha=%r must be finite and > 0' % (alpha,))
        self.model = model
        self.alpha = float(alpha)
        object.__setattr__(self, '_lam', None)           # not registered: out of state_dict(); follows the inputs' device

    def draw(self):
        """one lam ~ Beta(alpha, alpha) as float32, by the reference's call on numpy's global generator (trainer.py:162)"""
        return np.float32(np.random.beta(self.alpha, self.alpha, size=(1))[0])

    def lam_buffer(self, device):
        """the persistent one-element f32 device buffer forward() mixes with unless it is handed a tensor"""
        buf = self._lam
        if buf is None or buf.device != torch.device(device):
            buf = torch.zeros(1, dtype=torch.float32, device=device)
            object.__setattr__(self, '_lam', buf)
        return buf

    def set_lambda(self, value, device):
        """write a host value into lam_buffer(device) with a non-blocking copy from pinned memory; returns the buffer"""
        buf = self.lam_buffer(device)
        host = torch.tensor([float(np.float32(value))], dtype=torch.float32)
        buf.copy_(host.pin_memory() if buf.is_cuda else host, non_blocking=True)
        return buf

    def _lam_of(self, lam, device):
        if torch.is_tensor(lam):
            if lam.numel() != 1 or lam.dtype != torch.float32 or lam.device != device:
                raise ValueError('MixSpeechTraining: a lam tensor must be one f32 element on %s, got %s %s on %s'
                                 % (device, tuple(lam.shape), lam.dtype, lam.device))
            return lam.detach().reshape(1)
        return self.set_lambda(self.draw() if lam is None else lam, device)

    def forward(self, inputs, targets, lam=None):
        model = self.model
        if not self.training:
            return model(inputs, targets)
        x = inputs['inputs']
        if x.dim() != 3 or x.shape[0] < 2:
            raise ValueError('MixSpeechTraining: a batch of at least 2 utterances [B, T, F] is needed to form a pair, got %s' % (tuple(x.shape),))
        B = x.shape[0] // 2 * 2
        lam = self._lam_of(lam, x.device)
        lengths = inputs.get('inputs_length')
        if lengths is None:
            lengths = torch.sum(inputs['mask'], dim=-1)
        mixed, _, mixed_mask = ops.mixspeech_mix(x, lengths, lam)
        sets = [{key: t[k:B:2] for key, t in targets.items()} for k in (0, 1)]         # strided views: nothing is copied
        lam0 = lam.reshape(())
        om0 = 1 - lam0
        # a SpeechToText marks its memory: decoder and losses finish their backward before the encoder's starts (dp.py)
        memory, memory_mask = model.encode(mixed, mixed_mask, mark=isinstance(model, SpeechToText))
        aux = {'Lambda': lam0.detach()}
        if isinstance(model, SpeechToText):
            outs = [model.teacher_forced(memory, memory_mask, t, ctc=False) for t in sets]
            loss = lam0 * outs[0].ce + om0 * outs[1].ce
            loss_1, loss_2 = outs[0].ce.detach(), outs[1].ce.detach()
            if model.ctc_weight > 0:
                w = model.ctc_weight
                ctc_logits = model.assistor(memory, return_logits=True)
                ctc, ctc_1, ctc_2 = ops.ctc_loss_pair(ctc_logits, outs[0].target_out, outs[1].target_out, torch.sum(memory_mask, dim=-1),
                                                      sets[0]['targets_length'], sets[1]['targets_length'], lam, model.assistor.blank)
                loss = (1 - w) * loss + w * ctc
                loss_1, loss_2 = (1 - w) * loss_1 + w * ctc_1, (1 - w) * loss_2 + w * ctc_2
                aux['CTCLoss'] = ctc.detach()
        else:
            labels = [t['targets'][:, 1:-1] for t in sets]
            ctc_logits = model.assistor(memory, return_logits=True)
            loss, loss_1, loss_2 = ops.ctc_loss_pair(ctc_logits, labels[0], labels[1], torch.sum(memory_mask, dim=-1),
                                                     sets[0]['targets_length'].add(-1), sets[1]['targets_length'].add(-1), lam,
                                                     model.assistor.blank)
            aux['CTCLoss'] = loss.detach()
        aux['Loss_1'], aux['Loss_2'] = loss_1, loss_2
        return self.scale_loss_grad(loss), aux
