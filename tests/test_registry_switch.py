"""CPU (-m "not gpu"): INTEGRATION.md section 4 -- the drop-in classes stand in for the reference's.  Constructor and forward /
inference signatures of every drop-in equal the reference class's; parameter names and shapes of the model built from the yaml
dict are identical, so a reference checkpoint loads strict=True.  What the reference's classes look like is stored in
tests/golden/registry_switch.json (oracle/make_golden.py `registry` records it from the reference tree), so these checks need
nothing outside the repository.  Where the reference tree is present (REF), the fixture is checked against it and the switch is
also EXECUTED: the reference's own registries (otrans/frontend/__init__.py:8-12, encoder/__init__.py:10-13,
decoder/__init__.py:8-10) are pointed at the drop-in classes and the UNMODIFIED otrans.model.SpeechToText / CTCModel
(model/speech2text.py:19-23, model/ctc.py:72-79) build the HIP-backed model.  No compute is run (the product has no CPU path)."""
import importlib
import inspect
import json
import os
import sys

import pytest
import torch

from opentransformer_amd import synthetic as syn

REF = '/root/reference'
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'registry_switch.json')


def reference_package():
    """the reference's `otrans` package when its tree is present, else None"""
    if not os.path.isdir(os.path.join(REF, 'otrans')):
        return None
    for p in (os.path.join(REF, 'otrans', 'module'), REF):     # the first entry only serves `from activation import Swish` (otrans/module/ffn.py:9)
        if p not in sys.path:
            sys.path.insert(0, p)
    import otrans as pkg
    import otrans.model                                          # noqa: F401
    return pkg


@pytest.fixture(scope='module')
def otrans():
    return reference_package()


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _default(v):
    """a parameter default as JSON: no default, a tuple and anything that is not a JSON scalar or list are tagged"""
    if v is inspect.Parameter.empty:
        return {'empty': True}
    if isinstance(v, tuple):
        return {'tuple': [_default(x) for x in v]}
    if isinstance(v, list):
        return [_default(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return {'repr': repr(v)}


def signature_record(fn):
    """[name, kind, default] of every parameter (annotations / return types ignored), as stored in the fixture"""
    return [[p.name, p.kind.name, _default(p.default)] for p in inspect.signature(fn).parameters.values()]


def state_dict_record(model):
    """{key: shape} of a model's state_dict and the groups of keys that share one tensor (tied weights)"""
    sd = model.state_dict()
    by_ptr = {}
    for k, v in sd.items():
        by_ptr.setdefault(v.data_ptr(), []).append(k)
    return {'shapes': {k: list(v.shape) for k, v in sd.items()}, 'tied': sorted(g for g in by_ptr.values() if len(g) > 1)}


PAIRS = [  # (reference module path, class name, methods whose signature a caller relies on)
    ('otrans.frontend.conv', 'ConvFrontEnd', ('__init__', 'forward', 'inference')),
    ('otrans.encoder.transformer', 'TransformerEncoder', ('__init__', 'forward')),
    ('otrans.encoder.transformer', 'TransformerEncoderLayer', ('__init__', 'forward')),
    ('otrans.encoder.conformer', 'ConformerEncoder', ('__init__', 'forward')),
    ('otrans.decoder.transformer', 'TransformerDecoder', ('__init__', 'forward', 'inference')),
    ('otrans.decoder.transformer', 'TransformerDecoderLayer', ('__init__',)),
    ('otrans.module.attention', 'MultiHeadedSelfAttention', ('__init__',)),
    ('otrans.module.attention', 'MultiHeadedCrossAttention', ('__init__',)),
    ('otrans.module.ffn', 'PositionwiseFeedForward', ('__init__',)),
    ('otrans.module.loss', 'LabelSmoothingLoss', ('__init__', 'forward')),
    ('otrans.model.speech2text', 'SpeechToText', ('__init__', 'forward', 'save_checkpoint', 'load_model')),
    ('otrans.model.ctc', 'CTCModel', ('__init__', 'forward', 'save_checkpoint', 'set_epoch')),
    ('otrans.model.ctc', 'CTCAssistor', ('__init__', 'forward', 'compute_logits', 'compute_loss', 'inference')),
]

# the yaml dicts whose reference models the fixture describes
CONFIGS = {'c1_ctc': lambda: syn.c1_model(0.1, ctc_weight=0.3), 'conformer_ctc': lambda: syn.conformer_model(True, 0.1)}


@pytest.mark.parametrize('modpath,cls,methods', PAIRS)
def test_dropin_signatures_equal_the_reference(recorded, otrans, modpath, cls, methods):
    import opentransformer_amd as ota
    import opentransformer_amd.nn as onn
    mine = getattr(ota, cls, None) or getattr(onn, cls)
    for m in methods:
        key = '%s.%s.%s' % (modpath, cls, m)
        a = recorded['signatures'][key]
        if otrans is not None:                                   # the fixture still says what the reference tree says
            assert signature_record(getattr(getattr(importlib.import_module(modpath), cls), m)) == a, key
        b = signature_record(getattr(mine, m))
        if m == 'forward' and cls in ('TransformerEncoderLayer',):
            b = [p for p in b if p[0] != 'causal']                # one extra keyword with a default: callers of the reference never pass it
        assert [p[0] for p in a] == [p[0] for p in b], (cls, m, a, b)
        for pa, pb in zip(a, b):
            assert pa == pb, (cls, m, pa, pb)                     # kind and default


def test_registry_switch_builds_the_dropin_model_inside_the_reference(recorded, otrans):
    import opentransformer_amd as ota
    from opentransformer_amd._lib import OtransHipError
    cfg = CONFIGS['c1_ctc']()
    ref = recorded['state_dicts']['c1_ctc']
    hip_model = ota.SpeechToText(cfg)
    assert type(hip_model.frontend) is ota.ConvFrontEnd and type(hip_model.encoder) is ota.TransformerEncoder
    assert type(hip_model.decoder) is ota.TransformerDecoder
    # identical parameter names / shapes as the reference model built from the same yaml dict
    assert state_dict_record(hip_model)['shapes'] == ref['shapes']
    # a checkpoint in the reference's layout (speech2text.py save_checkpoint: one state_dict per part, the CTC head under 'ctc';
    # tied weights are one tensor) loads strict=True
    flat = {k: torch.empty(v) for k, v in ref['shapes'].items()}
    for group in ref['tied']:
        for k in group[1:]:
            flat[k] = flat[group[0]]
    syn.fill_state_dict_(flat, 4321)
    part_of = {'frontend': 'frontend', 'encoder': 'encoder', 'decoder': 'decoder', 'assistor': 'ctc'}
    chk = {}
    for k, v in flat.items():
        head, rest = k.split('.', 1)
        chk.setdefault(part_of[head], {})[rest] = v
    hip_model.load_model(chk)
    got = hip_model.state_dict()
    for k, v in flat.items():
        if not k.startswith('assistor.'):                        # the reference's load_model leaves the CTC head alone (speech2text.py:84-87)
            assert torch.equal(v, got[k]), k
    # the Conformer encoder (conformer_baseline.yaml's keys) behind the same constructor
    cm = ota.SpeechToText(CONFIGS['conformer_ctc']())
    assert type(cm.encoder) is ota.ConformerEncoder
    assert state_dict_record(cm)['shapes'] == recorded['state_dicts']['conformer_ctc']['shapes']
    # and there is no CPU fallback: compute on CPU tensors raises
    inputs, targets = syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=cfg['decoder']['vocab_size'],
                                          tgt_len=4, seed=0)
    with pytest.raises((OtransHipError, OSError, RuntimeError)):
        hip_model(inputs, targets)
    if otrans is not None:
        _switch_inside_the_reference(otrans, recorded)


def _switch_inside_the_reference(otrans, recorded):
    """INTEGRATION.md section 4 executed inside the reference tree; the fixture is checked against the reference models"""
    import opentransformer_amd as ota
    from opentransformer_amd._lib import OtransHipError
    import otrans.frontend as rf
    import otrans.encoder as re_
    import otrans.decoder as rd
    import otrans.model.speech2text as rs2t
    cfg = CONFIGS['c1_ctc']()
    ref_model = otrans.model.End2EndModel['speech2text'](cfg)                # the reference as shipped
    assert state_dict_record(ref_model) == recorded['state_dicts']['c1_ctc']
    assert state_dict_record(otrans.model.End2EndModel['speech2text'](CONFIGS['conformer_ctc']())) == recorded['state_dicts']['conformer_ctc']
    saved = (dict(rf.BuildFrontEnd), dict(re_.BuildEncoder), dict(rd.BuildDecoder))
    try:
        # ---- INTEGRATION.md section 4, verbatim
        rf.BuildFrontEnd['conv'] = ota.ConvFrontEnd
        re_.BuildEncoder['transformer'] = ota.TransformerEncoder
        re_.BuildEncoder['conformer'] = ota.ConformerEncoder
        rd.BuildDecoder['transformer'] = ota.TransformerDecoder
        # the reference's model files bound the registries by name at import: they are the same dict objects
        assert rs2t.BuildFrontEnd is rf.BuildFrontEnd and rs2t.BuildEncoder is re_.BuildEncoder and rs2t.BuildDecoder is rd.BuildDecoder
        hip_model = otrans.model.End2EndModel['speech2text'](cfg)            # UNMODIFIED otrans.model.SpeechToText
        assert type(hip_model) is rs2t.SpeechToText
        assert type(hip_model.frontend) is ota.ConvFrontEnd and type(hip_model.encoder) is ota.TransformerEncoder
        assert type(hip_model.decoder) is ota.TransformerDecoder
        # identical parameter names / shapes: the reference's checkpoint dict loads strict=True through its own load_model()
        a = {k: tuple(v.shape) for k, v in ref_model.state_dict().items()}
        b = {k: tuple(v.shape) for k, v in hip_model.state_dict().items()}
        assert a == b
        chk = {'frontend': ref_model.frontend.state_dict(), 'encoder': ref_model.encoder.state_dict(),
               'decoder': ref_model.decoder.state_dict(), 'ctc': ref_model.assistor.state_dict()}
        hip_model.load_model(chk)
        for (k, v), (_, w) in zip(sorted(ref_model.state_dict().items()), sorted(hip_model.state_dict().items())):
            if not k.startswith('assistor.'):                    # the reference's load_model leaves the CTC head alone (speech2text.py:84-87)
                assert torch.equal(v, w), k
        # the same through the CTC model and the Conformer encoder (conformer_baseline.yaml's keys)
        ccfg = CONFIGS['conformer_ctc']()
        cm = otrans.model.End2EndModel['speech2text'](ccfg)
        assert type(cm.encoder) is ota.ConformerEncoder
        # and there is no CPU fallback hiding behind the switch: compute on CPU tensors raises
        inputs, targets = syn.synthetic_batch(batch=2, frames=64, feat_dim=cfg['frontend']['input_size'], vocab=cfg['decoder']['vocab_size'],
                                              tgt_len=4, seed=0)
        with pytest.raises((OtransHipError, OSError, RuntimeError)):
            hip_model(inputs, targets)
    finally:
        for reg, old in zip((rf.BuildFrontEnd, re_.BuildEncoder, rd.BuildDecoder), saved):
            reg.clear()
            reg.update(old)
