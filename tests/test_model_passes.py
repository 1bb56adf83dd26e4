"""The pieces every training objective is composed of (opentransformer_amd/model.py): shift_targets, AcousticModel.encode,
teacher_forced, evaluating and the ModelTraining base of MWERTraining and DistillTraining.  CPU (-m "not gpu"): what can be said without a
device -- the target views, that every pass goes through the one encode step, the restored modes, the delegation.  GPU: the wrappers
report the loss the model's own forward() reports."""
import copy

import pytest
import torch
import torch.nn as nn

import opentransformer_amd as ota
from opentransformer_amd import model as M
from opentransformer_amd import synthetic as syn

DEV = 'cuda'


# ---------------------------------------------------------------- shift_targets
def _truths():
    plain = torch.arange(1, 25).view(4, 6)
    strided = torch.arange(1, 25).view(6, 4).t()            # [4, 6] with inner stride 4
    assert strided.stride(-1) != 1
    return {'plain': plain, 'strided': strided}


@pytest.mark.parametrize('stacked', [False, True])
@pytest.mark.parametrize('kind', ['plain', 'strided'])
def test_shift_targets_values_and_stacked_form(kind, stacked):
    truth = _truths()[kind]
    dec_in, target_out = M.shift_targets(truth, stacked)
    assert torch.equal(dec_in, truth[:, :-1]) and torch.equal(target_out, truth[:, 1:])
    # not on the device (and, for one of the two, no unit inner stride): the stacked form whatever the flag says -- one new buffer
    # that holds both halves, contiguous, and nothing of the target matrix itself
    own = dec_in.untyped_storage().data_ptr()
    assert own == target_out.untyped_storage().data_ptr() != truth.untyped_storage().data_ptr()
    assert dec_in.is_contiguous() and target_out.is_contiguous()
    assert target_out.data_ptr() - dec_in.data_ptr() == dec_in.numel() * dec_in.element_size()


# ---------------------------------------------------------------- one encode step
class _Reached(Exception):
    pass


def _batch(cfg):
    return syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=cfg['decoder']['vocab_size'], tgt_len=4,
                               seed=0)


def _s2t(ctc_weight=0.3):
    cfg = syn.c1_model(0.0, ctc_weight=ctc_weight)
    return ota.SpeechToText(cfg), cfg


def _ctc():
    cfg = syn.c1_model(0.0)
    return ota.CTCModel(dict(cfg, vocab_size=cfg['decoder']['vocab_size'])), cfg


def _forward(model, cfg):
    return lambda: model(*_batch(cfg))


def _with_labels(method, cfg):
    inputs, targets = _batch(cfg)
    return lambda: method(inputs['inputs'], inputs['mask'], targets['targets'][:, 1:-1], targets['targets_length'] - 1)


def _entries():
    """name -> a call on CPU tensors that has to arrive at the encode step before anything touches a device"""
    s2t, cfg = _s2t()
    ctc, ccfg = _ctc()
    inputs, targets = _batch(cfg)
    V = cfg['decoder']['vocab_size']
    stored = {'att': torch.zeros(2, targets['targets'].shape[1] - 1, V), 'ctc': torch.zeros(2, 15, V)}
    return {
        'SpeechToText.forward': _forward(s2t, cfg),
        'SpeechToText.forward without CTC': _forward(*_s2t(0.0)),
        'SpeechToText.align': _with_labels(s2t.align, cfg),
        'CTCModel.forward': _forward(ctc, ccfg),
        'CTCModel.inference': lambda: ctc.inference(inputs['inputs'], inputs['mask']),
        'CTCModel.align': _with_labels(ctc.align, ccfg),
        'DistillTraining.forward from stored outputs': lambda: ota.DistillTraining(s2t)(inputs, targets, teacher_out=stored),
        'DistillTraining.forward of a CTCModel from stored outputs': lambda: ota.DistillTraining(ctc)(inputs, targets, teacher_out=stored),
        'DistillTraining.teacher_outputs': lambda: ota.DistillTraining(s2t, copy.deepcopy(s2t)).teacher_outputs(inputs, targets),
        'DistillTraining.teacher_outputs of a CTCModel': lambda: ota.DistillTraining(ctc, copy.deepcopy(ctc)).teacher_outputs(inputs, targets),
    }


@pytest.mark.parametrize('entry', sorted(_entries()))
def test_every_pass_goes_through_the_one_encode_step(monkeypatch, entry):
    seen = []

    def spy(self, inputs, inputs_mask, mark=False):
        seen.append((type(self).__name__, mark))
        raise _Reached()
    monkeypatch.setattr(M.AcousticModel, 'encode', spy)
    with pytest.raises(_Reached):
        _entries()[entry]()
    # the early mark belongs to the SpeechToText training passes; CTCModel, the alignments and the teacher pass never place it
    marked = entry.startswith(('SpeechToText.forward', 'DistillTraining.forward from'))
    assert seen == [('CTCModel' if 'CTCModel' in entry else 'SpeechToText', marked)]


# ---------------------------------------------------------------- evaluating
def _toy():
    tree = nn.Sequential(nn.Linear(2, 2), nn.Sequential(nn.Dropout(0.5), nn.Linear(2, 2)), nn.Dropout(0.1))
    tree.train()
    tree[1].eval()
    tree[1][1].train()
    tree[2].eval()
    return tree


def test_evaluating_restores_a_mixed_set_of_modes():
    tree = _toy()
    before = [m.training for m in tree.modules()]
    assert len(set(before)) == 2
    with M.evaluating(tree) as inside:
        assert inside is tree and not any(m.training for m in tree.modules())
    assert [m.training for m in tree.modules()] == before
    with pytest.raises(_Reached):
        with M.evaluating(tree):
            assert not any(m.training for m in tree.modules())
            raise _Reached()
    assert [m.training for m in tree.modules()] == before


# ---------------------------------------------------------------- the ModelTraining base
class _Recording(ota.SpeechToText):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.calls = []

    def save_checkpoint(self, params, name):
        self.calls.append(('save_checkpoint', params, name))

    def load_model(self, chkpt):
        self.calls.append(('load_model', chkpt))

    def set_epoch(self, epoch):
        self.calls.append(('set_epoch', epoch))


@pytest.mark.parametrize('wrapper', ['mwer', 'distill'])
def test_wrappers_are_model_trainings(wrapper):
    model = _Recording(syn.c1_model(0.0, ctc_weight=0.3)).train()
    modes = [m.training for m in model.modules()]
    if wrapper == 'mwer':
        wrap = ota.MWERTraining(model, nbest=2, recognizer=object())
    else:
        wrap = ota.DistillTraining(model, copy.deepcopy(model))
    assert isinstance(wrap, M.ModelTraining) and wrap.model is model
    assert [m.training for m in model.modules()] == modes
    names = [n for n, _ in wrap.named_parameters()]
    assert names == ['model.' + n for n, _ in model.named_parameters()] and len(names) > 10
    assert list(wrap.state_dict()) == ['model.' + k for k in model.state_dict()]
    wrap.save_checkpoint({'p': 1}, 'name.pt')
    wrap.load_model({'frontend': {}})
    wrap.set_epoch(3)
    assert model.calls == [('save_checkpoint', {'p': 1}, 'name.pt'), ('load_model', {'frontend': {}}), ('set_epoch', 3)]


# ---------------------------------------------------------------- GPU: one loss, whoever asks for it
CTC_SLACK = 4 * 2.0 ** -23     # two passes of otr_ctc_loss: it adds its B terms with floating-point atomics (tests/test_gpu_distill.py)


@pytest.mark.gpu
@pytest.mark.parametrize('ctc_weight', [0.0, 0.3])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_wrappers_report_the_models_own_loss(mode, ctc_weight):
    """C1, batch 2, 64 frames, 4 target tokens, no dropout.  MWERTraining's 'CE' is the model's cross-entropy on targets read in place,
    DistillTraining's 'Loss' the model's own loss, both from the pass forward() runs: bit-equal to what forward() returns.  With a CTC
    term forward() reports the mix and the CTC part; the cross-entropy (stacked targets in forward() and the distillation step, read in
    place in the MWER step) is compared bit for bit through the mix formed from it, the CTC part within CTC_SLACK, relative."""
    from opentransformer_amd import ops
    try:
        ops.set_compute_dtype(mode)
        model, cfg = _s2t(ctc_weight)
        syn.fill_state_dict_(model.state_dict(), 1234)
        model = model.to(DEV).train()
        inputs, targets = _batch(cfg)
        inputs = {k: v.to(DEV) for k, v in inputs.items()}
        targets = {k: v.to(DEV) for k, v in targets.items()}
        truth, n = targets['targets'], targets['targets_length'] - 1
        tokens = truth[:, 1:].unsqueeze(1).repeat(1, 2, 1)      # slot 0: the reference; slot 1: its first token replaced
        tokens[:, 1, 0] = 2 + (tokens[:, 1, 0] + 5) % (cfg['decoder']['vocab_size'] - 2)
        hyps = (tokens, n.to(torch.int32).unsqueeze(1).repeat(1, 2))
        loss, aux = model(inputs, targets)
        _, mwer = ota.MWERTraining(model, nbest=2, ce_weight=0.01)(inputs, targets, hyps=hyps)
        _, kd = ota.DistillTraining(model, copy.deepcopy(model), kd_weight=0.5)(inputs, targets)
        torch.cuda.synchronize()
        print('model passes %s ctc_weight %g: forward %.9g, MWER CE %.9g, distill Loss %.9g' % (
            mode, ctc_weight, loss.item(), mwer['CE'].item(), kd['Loss'].item()))
        assert model.training and loss.item() > 0
        if ctc_weight == 0:
            assert aux is None and 'CTCLoss' not in kd
            assert torch.equal(mwer['CE'], loss.detach())
            assert torch.equal(kd['Loss'], loss.detach())
        else:
            print('  CTC part: forward %.9g, distill %.9g' % (aux['CTCLoss'].item(), kd['CTCLoss'].item()))
            ce = mwer['CE']
            assert torch.equal((1 - ctc_weight) * ce + ctc_weight * aux['CTCLoss'], loss.detach())
            assert torch.equal((1 - ctc_weight) * ce + ctc_weight * kd['CTCLoss'], kd['Loss'])
            assert abs(kd['CTCLoss'].item() - aux['CTCLoss'].item()) <= CTC_SLACK * abs(aux['CTCLoss'].item())
    finally:
        ops.set_compute_dtype('bf16')
