"""CPU (-m "not gpu"): feature preparation for device batch assembly.  The numpy float64 restatement (tests/feature_prepare_ref.py)
equals the reference's chain (tests/golden/feature_chain.npz, written by tests/make_feature_golden.py from the reference's own
spec_augment and the restated lines of otrans/data/audio.py), FeaturePipeline draws on the host in the reference's order, GlobalCMVN
round-trips its two files, and the entry points refuse what include/otrans_hip.h says they refuse before any launch."""
import ctypes as C
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, data, ops
from tests import feature_prepare_ref as ref

ROOT = Path(__file__).resolve().parent.parent
SPEC_DEFAULT = dict(freq_mask_num=2, time_mask_num=2, freq_mask_rate=0.3, time_mask_rate=0.05)    # spec_augment's own defaults


@pytest.fixture(scope='module')
def chain(golden):
    return golden('feature_chain.npz')


def _seed(g):
    torch.manual_seed(int(g['seed']))
    np.random.seed(int(g['seed']))
    random.seed(int(g['seed']))


def _pipeline(g, **kw):
    params = dict(normalization=True, gaussian_noise=float(g['sigma']), spec_augment=True, spec_augment_config=SPEC_DEFAULT)
    params.update(kw)
    return data.FeaturePipeline(params)


def test_restatement_equals_the_reference_normalisation(chain):
    """float32 torch.std_mean against float64: inside the 1x bound the GPU tests allow twice of"""
    for b in range(3):
        x = chain['x%d' % b]
        mean, std = ref.utterance_stats(x)
        y = ref.chain(x, 'utterance')
        assert np.all(np.abs(chain['norm_utt%d' % b] - y) <= ref.EPS32 * (np.abs(y) + abs(mean) / std + 1))
        y = ref.chain(x, 'global', chain['gmean'], chain['gstd'])
        assert np.all(np.abs(chain['norm_glob%d' % b] - y) <= ref.EPS32 * (np.abs(y) + 1))


def test_global_statistics_of_the_fixture_are_the_population_ones(chain):
    mean, std = ref.cmvn_result(ref.cmvn_sums([chain['x%d' % b] for b in range(3)]))
    np.testing.assert_allclose(mean, chain['gmean'], rtol=1e-6)
    np.testing.assert_allclose(std, chain['gstd'], rtol=1e-6)


@pytest.mark.parametrize('norm', ['utterance', 'global'])
def test_host_draws_and_restated_chain_equal_the_reference(chain, norm):
    """FeaturePipeline.draw under the fixture's seeds: the reference's noise bit for bit, and rectangles that zero exactly the cells
    the reference's spec_augment zeroed; the restated chain on those draws is the reference's output to float32 rounding"""
    key = 'chain_utt%d' if norm == 'utterance' else 'chain_glob%d'
    lengths = [int(v) for v in chain['lengths']]
    _seed(chain)
    noise, rows = _pipeline(chain).draw(lengths, 8)
    assert noise.shape == (3, 8) and len(rows) == 3 and all(len(r) == 4 for r in rows)
    for b in range(3):
        assert np.array_equal(noise[b].numpy(), chain['noise%d' % b])
        y = ref.chain(chain['x%d' % b], norm, chain['gmean'], chain['gstd'], noise[b].numpy(), rows[b])
        want = chain[key % b]
        assert np.array_equal(y == 0, want == 0) and (want == 0).any()
        mean, std = ref.utterance_stats(chain['x%d' % b])
        assert np.all(np.abs(want - y) <= 2 * ref.EPS32 * (np.abs(y) + (abs(mean) / std if norm == 'utterance' else 0) + 1))
    packed = ref.prepare([chain['x%d' % b] for b in range(3)], 40, norm, chain['gmean'], chain['gstd'], noise.numpy(), rows)
    assert packed['mask'].sum(1).tolist() == lengths and not packed['dst'][1, 23:].any() and not packed['bound'][1, 23:].any()
    assert np.array_equal(packed['dst'] == 0, ref.zero_cells(lengths, 40, 8, rows))


def test_eval_and_switched_off_stages_draw_nothing(chain):
    params = dict(normalization=True, gaussian_noise=0.3, spec_augment=True, spec_augment_config=SPEC_DEFAULT)
    _seed(chain)
    state = (torch.get_rng_state().clone(), np.random.get_state()[1].copy(), random.getstate())
    ev = data.FeaturePipeline(params, is_eval=True)
    assert ev.norm == 'utterance' and ev.draw([30, 20], 8) == (None, None)
    off = data.FeaturePipeline(dict(normalization=False, gaussian_noise=0.0, spec_augment=False))
    assert off.norm is None and off.draw([30, 20], 8) == (None, None)
    assert torch.equal(torch.get_rng_state(), state[0]) and np.array_equal(np.random.get_state()[1], state[1])
    assert random.getstate() == state[2]
    # noise only: no numpy / random draw;  SpecAugment only: no torch draw
    data.FeaturePipeline(dict(normalization=False, gaussian_noise=0.3, spec_augment=False)).draw([30], 8)
    assert np.array_equal(np.random.get_state()[1], state[1]) and not torch.equal(torch.get_rng_state(), state[0])


def test_pipeline_refuses_an_empty_utterance():
    batch = [('a', torch.zeros(4, 8), 4, [3], 1), ('b', torch.zeros(0, 8), 0, [4], 1)]
    with pytest.raises(ValueError, match="'b'"):
        data.FeaturePipeline(dict(normalization=True, spec_augment=False))(batch)


def test_global_cmvn_files_round_trip(chain, tmp_path):
    utts = [chain['x%d' % b] for b in range(3)]
    cm = data.GlobalCMVN(8, 'cpu')
    cm.acc.copy_(torch.from_numpy(ref.cmvn_sums(utts)))
    mean, std = cm.result()
    assert mean.dtype == torch.float32 and std.dtype == torch.float32
    allx = np.concatenate(utts).astype(np.float64)
    np.testing.assert_allclose(mean.numpy(), allx.mean(0), rtol=1e-6)
    np.testing.assert_allclose(std.numpy(), allx.std(0), rtol=1e-6)
    prefix = str(tmp_path / 'cmvn')
    cm.save(prefix)
    assert sorted(p.name for p in tmp_path.iterdir()) == ['cmvn.mean.npy', 'cmvn.std.npy']
    m2, s2 = data.GlobalCMVN.load(prefix)
    assert torch.equal(m2, mean) and torch.equal(s2, std)
    pipe = data.FeaturePipeline(dict(normalization=True, global_cmvn=prefix, spec_augment=False))    # the keys audio.py:43-45 reads
    assert pipe.norm == 'global' and torch.equal(pipe.gmean, mean) and torch.equal(pipe.gstd, std)
    with pytest.raises(_lib.OtransHipError):
        cm.update(torch.zeros(4, 8), torch.zeros(1, dtype=torch.int64), torch.full((1,), 4, dtype=torch.int32))


def test_entries_are_declared_bound_and_exported():
    """additions only: the ABI number stays where the existing bindings expect it, the three entries are in the header, the binding
    and both libraries"""
    header = (ROOT / 'include' / 'otrans_hip.h').read_text()
    assert int(re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1)) == _lib.OTR_ABI_VERSION
    for name in ('otr_feature_prepare_workspace_bytes', 'otr_feature_prepare', 'otr_cmvn_accumulate'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SIGNATURES
        for kind in ('bf16', 'fp16'):
            lib = _lib.load(kind)
            assert lib.otr_version() == _lib.OTR_ABI_VERSION and hasattr(lib, name)


def test_workspace_size_and_refused_shapes():
    lib = _lib.load()
    assert lib.otr_feature_prepare_workspace_bytes(32, 1000, 80) == 32 * (1 + 2 * 20) * 8      # 80000 values = 20 chunks of 4096
    assert lib.otr_feature_prepare_workspace_bytes(1, 1, 1) == 24
    assert lib.otr_feature_prepare_workspace_bytes(0, 5, 5) == 0
    for B, Tmax, F in ((-1, 10, 8), (4, 0, 8), (4, 10, 0), (4, -3, 8), (65536, 10, 8), (4, 1 << 20, 1 << 11)):
        assert lib.otr_feature_prepare_workspace_bytes(B, Tmax, F) == -1, (B, Tmax, F)


def test_entry_points_refuse_bad_arguments_and_leave_the_outputs_alone():
    """checked on the host before any launch (no GPU needed): every output buffer still holds its fill afterwards"""
    lib = _lib.load()
    fill = 123.25
    bufs = {k: (C.c_float * 256)(*([fill] * 256)) for k in ('dst', 'mask', 'stats', 'ws', 'acc')}
    p = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}
    inp = C.cast((C.c_float * 256)(), C.c_void_p)

    def call(src=inp, row_off=inp, lengths=inp, B=2, Tmax=5, F=4, mode=1, gmean=inp, gstd=inp, noise=inp, ranges=inp, NR=2,
             dst=p['dst'], mask=p['mask'], stats=p['stats'], ws=p['ws'], nws=1024):
        return lib.otr_feature_prepare(src, row_off, lengths, B, Tmax, F, mode, gmean, gstd, noise, ranges, NR, dst, mask, stats, ws,
                                       nws, None)
    bad = [dict(src=None), dict(row_off=None), dict(lengths=None), dict(dst=None), dict(B=-1), dict(Tmax=0), dict(F=0), dict(NR=-1),
           dict(NR=65), dict(NR=1, ranges=None), dict(mode=-1), dict(mode=3), dict(mode=2, gmean=None), dict(mode=2, gstd=None),
           dict(nws=2 * 3 * 8 - 1), dict(ws=None)]
    for kw in bad:
        assert call(**kw) < 0, kw
        msg = lib.otr_last_error_string()
        assert msg and b'feature_prepare' in msg, (kw, msg)
    assert lib.otr_cmvn_accumulate(None, inp, inp, 2, 4, p['acc'], None) < 0
    assert lib.otr_cmvn_accumulate(inp, None, inp, 2, 4, p['acc'], None) < 0
    assert lib.otr_cmvn_accumulate(inp, inp, None, 2, 4, p['acc'], None) < 0
    assert lib.otr_cmvn_accumulate(inp, inp, inp, 2, 4, None, None) < 0
    assert lib.otr_cmvn_accumulate(inp, inp, inp, -1, 4, p['acc'], None) < 0
    assert lib.otr_cmvn_accumulate(inp, inp, inp, 2, 0, p['acc'], None) < 0
    assert b'cmvn_accumulate' in lib.otr_last_error_string()
    assert call(B=0) == 0 and lib.otr_cmvn_accumulate(inp, inp, inp, 0, 4, p['acc'], None) == 0      # nothing to do, no launch
    for k, v in bufs.items():
        assert all(x == fill for x in v), k


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    src, ro, ln = torch.zeros(6, 4), torch.zeros(2, dtype=torch.int64), torch.full((2,), 3, dtype=torch.int32)
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):
        ops.feature_prepare(src, ro, ln, 3, norm='utterance')
    with pytest.raises(_lib.OtransHipError, match='no CPU fallback'):
        ops.cmvn_accumulate(src, ro, ln, torch.zeros(9, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.feature_prepare(src, ro, ln, 3, norm='cmvn')
    with pytest.raises(ValueError):
        ops.feature_prepare(src, ro, ln, 3, norm='global')
