"""Knowledge distillation of a SpeechToText or CTCModel student from a teacher of the same class on the device (Hinton et al. 2015;
include/otrans_hip.h otr_distill_loss): the temperature-scaled KL divergence of the student's logits from the teacher's, per head and
per frame, beside the student's own loss.  The teacher's posteriors come from a teacher pass inside the step (online) or from what
teacher_outputs() returned earlier (offline; with topk = K they are the K best entries per frame, 2K numbers instead of V).  The
working form of the reference's teacher-student hook (otrans/model/ctc.py:105-115 ts_forward)."""
import torch

from . import ops
from .model import CTCModel, ModelTraining, SpeechToText, shift_targets


def _vocab(model):
    head = model.decoder if isinstance(model, SpeechToText) else model.assistor
    return head.output_layer.weight.shape[0]


class DistillTraining(ModelTraining):
    """Wraps the student as the submodule `model` (FusedAdam / FlatDataParallel see the same parameters under `model.`);
    forward(inputs, targets, teacher_out=None) -> (loss, aux) with loss = (1 - kd_weight) * own + kd_weight * kd.

    own is the student's loss exactly as its forward() forms it.  A SpeechToText student: KD_att = ops.distill_loss on the
    teacher-forced decoder logits over the positions below targets_length; when student and teacher both have a CTC head, KD_ctc on
    the heads' logits over the frames below the memory length, and kd = (1 - ctc_weight) * KD_att + ctc_weight * KD_ctc (the student's
    ctc_weight), else kd = KD_att.  A CTCModel student: own is its CTC loss and kd = KD_ctc.  The two classes train their CTC heads on
    different label sequences, so the teacher must be of the student's class, with the same vocabulary and the same subsampling.

    The teacher runs in eval() under no_grad; it is NOT a submodule -- parameters(), state_dict() and modules() are the student's, and
    .to() / .train() leave it alone: place it on the device yourself.  teacher_outputs(inputs, targets) returns what a step needs of
    it, per head ('att', 'ctc'): the dense logits, or with topk = K the pair ops.topk_rows(logits, lengths, K).  Passing that dict as
    teacher_out skips the teacher pass (offline distillation; teacher=None is legal then, and a dict of either form is accepted).
    aux: 'Loss' (own), 'KD', 'KD_att', 'KD_ctc', and 'CTCLoss' where the student has a CTC head -- detached device scalars, no host
    synchronisation."""

    def __init__(self, model, teacher=None, kd_weight=0.5, temperature=2.0, topk=None):
        super().__init__()
        if not isinstance(model, (SpeechToText, CTCModel)):
            raise ValueError('DistillTraining: the student must be a SpeechToText or a CTCModel, got %s' % type(model).__name__)
        if not 0.0 <= float(kd_weight) <= 1.0:
            raise ValueError('DistillTraining: kd_weight=%r must be in [0, 1]' % (kd_weight,))
        if not (float(temperature) > 0.0 and float(temperature) != float('inf')):
            raise ValueError('DistillTraining: temperature=%r must be finite and > 0' % (temperature,))
        if topk is not None and not 1 <= int(topk) <= ops.DISTILL_MAX_K:
            raise ValueError('DistillTraining: topk=%r must be in [1, %d]' % (topk, ops.DISTILL_MAX_K))
        if teacher is not None:
            if type(teacher) is not type(model):
                raise ValueError('DistillTraining: the teacher is a %s, the student a %s: their CTC heads are trained on different label '
                                 'sequences, both must be of one class' % (type(teacher).__name__, type(model).__name__))
            if _vocab(teacher) != _vocab(model):
                raise ValueError('DistillTraining: the teacher\'s vocabulary V=%d differs from the student\'s V=%d' % (_vocab(teacher), _vocab(model)))
            teacher.eval()
        self.model = model
        object.__setattr__(self, 'teacher', teacher)      # not registered: out of parameters(), state_dict() and modules()
        self.kd_weight, self.temperature, self.topk = float(kd_weight), float(temperature), None if topk is None else int(topk)

    @torch.no_grad()
    def teacher_outputs(self, inputs, targets):
        """{'att': ..., 'ctc': ...} (the heads the teacher has): dense f32 logits, or (val, idx) of ops.topk_rows with topk = K"""
        teacher = self.teacher
        if teacher is None:
            raise ValueError('DistillTraining.teacher_outputs: there is no teacher')
        if teacher.training:                              # the teacher stays in eval(): nothing to put back, no walk over its modules per step
            teacher.eval()
        memory, memory_mask = teacher.encode(inputs['inputs'], inputs['mask'])
        heads = {}
        if isinstance(teacher, SpeechToText):
            dec_in, _ = shift_targets(targets['targets'])
            heads['att'] = (teacher.decoder(dec_in, memory, memory_mask)[0], targets['targets_length'])
        if getattr(teacher, 'assistor', None) is not None:
            heads['ctc'] = (teacher.assistor(memory, return_logits=True), torch.sum(memory_mask, dim=-1))
        if self.topk is None:
            return {k: logits for k, (logits, _) in heads.items()}
        return {k: ops.topk_rows(logits, lengths, self.topk) for k, (logits, lengths) in heads.items()}

    def _kd(self, head, logits, lengths, teacher_out):
        t = teacher_out[head]
        what = 'decoder positions L' if head == 'att' else 'encoder frames T\''
        shape = tuple(t[0].shape[:2]) if isinstance(t, (tuple, list)) else tuple(t.shape[:2])
        if shape[0] == logits.shape[0] and shape[1] != logits.shape[1]:
            raise ValueError('DistillTraining: the teacher has %d %s, the student %d' % (shape[1], what, logits.shape[1]))
        if isinstance(t, (tuple, list)):
            return ops.distill_loss_topk(logits, t[0], t[1], lengths, self.temperature)[0]
        if t.shape[-1] != logits.shape[-1]:
            raise ValueError('DistillTraining: the teacher\'s vocabulary V=%d differs from the student\'s V=%d' % (t.shape[-1], logits.shape[-1]))
        return ops.distill_loss(logits, t, lengths, self.temperature)[0]

    def forward(self, inputs, targets, teacher_out=None):
        model = self.model
        if teacher_out is None:
            if self.teacher is None:
                raise ValueError('DistillTraining.forward: neither a teacher nor teacher_out was given')
            teacher_out = self.teacher_outputs(inputs, targets)
        own_head = 'att' if isinstance(model, SpeechToText) else 'ctc'
        if own_head not in teacher_out:
            raise ValueError('DistillTraining: teacher_out has no \'%s\' entry for a %s student' % (own_head, type(model).__name__))
        # a SpeechToText student marks its memory: decoder and losses finish their backward before the encoder's starts (dp.py)
        memory, memory_mask = model.encode(inputs['inputs'], inputs['mask'], mark=isinstance(model, SpeechToText))
        out = model.teacher_forced(memory, memory_mask, targets)
        own, kd_att, kd_ctc = out.loss, None, None
        if out.logits is not None:
            kd = kd_att = self._kd('att', out.logits, targets['targets_length'], teacher_out)
        if out.ctc_logits is not None and 'ctc' in teacher_out:
            kd = kd_ctc = self._kd('ctc', out.ctc_logits, out.memory_length, teacher_out)
            if kd_att is not None:
                kd = (1 - model.ctc_weight) * kd_att + model.ctc_weight * kd_ctc
        total = (1 - self.kd_weight) * own + self.kd_weight * kd
        zero = torch.zeros_like(kd.detach())
        aux = {'Loss': own.detach(), 'KD': kd.detach(), 'KD_att': kd_att.detach() if kd_att is not None else zero,
               'KD_ctc': kd_ctc.detach() if kd_ctc is not None else zero}
        if out.ctc is not None:
            aux['CTCLoss'] = out.ctc.detach()
        return self.scale_loss_grad(total), aux
