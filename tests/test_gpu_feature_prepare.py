"""GPU (-m gpu): otr_feature_prepare / otr_cmvn_accumulate / ops.feature_prepare / data.FeaturePipeline / data.GlobalCMVN against the
numpy float64 restatement tests/feature_prepare_ref.py.  The entry is called directly where the outputs have to be pre-filled: dst and
stats with NaN, mask with 0xFF, the gaps of the packed buffer and the padding of the in-place one with NaN, so a cell that was not
written, or a value that should not have been read, shows.

Tolerance (derived, tests/feature_prepare_ref.py:prepare): |y - y64| <= 2 * 2^-23 * (|y64| + |mean| / std + 1) for utterance
normalisation, 2 * 2^-23 * (|y64| + 1) for global CMVN and the copy, 0 where the result is zero by construction; stats within 2^-23
relative.  A single-pass fp32 sum of squares misses the first by > 1000x on the large-offset data."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, data, ops
from tests import feature_prepare_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1401]
BATCHES = {1: [257], 3: [1401, 1, 64], 33: [LENGTHS[(7 * i + 3) % 10] for i in range(33)]}
MODES = {0: None, 1: 'utterance', 2: 'global'}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _batch(B, F, loc=3.0, scale=2.0):
    """the utterances of a case and their global statistics; made once, never modified"""
    rng = np.random.default_rng(1000 * B + F)
    utts = [(rng.standard_normal((T, F)) * scale * (1 + 0.1 * (b % 5)) + loc + 0.25 * np.arange(F)).astype(np.float32)
            for b, T in enumerate(BATCHES[B])]
    for u in utts:
        u.setflags(write=False)
    gmean, gstd = ref.cmvn_result(ref.cmvn_sums(utts))
    return utts, gmean.astype(np.float32), np.maximum(gstd, 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _want(B, F, mode):
    utts, gmean, gstd = _batch(B, F)
    return ref.prepare(utts, max(BATCHES[B]), MODES[mode], gmean, gstd)


def run_entry(utts, Tmax, mode, form='packed', gmean=None, gstd=None, noise=None, ranges=None, src_shift=0, dst_shift=0,
              gaps=(0, 1, 2, 3), lengths=None, want_mask=True, want_stats=True):
    """otr_feature_prepare on pre-filled buffers -> (dst [B, Tmax, F], mask uint8 [B, Tmax], stats [B, 2]) as numpy.
    packed: utterance b starts gaps[b % len(gaps)] frames after the end of the one before, inside a NaN-filled buffer whose first
    value sits src_shift floats past a 256-byte aligned address; dst likewise dst_shift floats.  inplace: src == dst [B, Tmax, F],
    NaN past each utterance, row_off = b * Tmax."""
    lib = _lib.load()
    B, F = len(utts), utts[0].shape[1]
    lens = [u.shape[0] for u in utts] if lengths is None else list(lengths)
    if form == 'packed':
        offs, cur = [], 0
        for b, u in enumerate(utts):
            cur += gaps[b % len(gaps)]
            offs.append(cur)
            cur += u.shape[0]
        host = np.full(src_shift + (cur + 1) * F, np.nan, np.float32)
        for o, u in zip(offs, utts):
            host[src_shift + o * F:src_shift + (o + u.shape[0]) * F] = u.reshape(-1)
        src = _dev(host)[src_shift:]
        dst = torch.full((dst_shift + B * Tmax * F,), float('nan'), dtype=torch.float32, device=DEV)[dst_shift:]
    else:
        host = np.full((B, Tmax, F), np.nan, np.float32)
        for b, u in enumerate(utts):
            host[b, :min(u.shape[0], Tmax)] = u[:Tmax]
        src = dst = torch.cat([torch.zeros(dst_shift), torch.from_numpy(host).reshape(-1)]).to(DEV)[dst_shift:]
        offs = [b * Tmax for b in range(B)]
    assert src.data_ptr() % 16 == (4 * (src_shift if form == 'packed' else dst_shift)) % 16
    mask = torch.full((B, Tmax), 0xFF, dtype=torch.uint8, device=DEV) if want_mask else None
    stats = torch.full((B, 2), float('nan'), dtype=torch.float32, device=DEV) if want_stats else None
    nws = lib.otr_feature_prepare_workspace_bytes(B, Tmax, F)
    assert nws >= 0
    ws = torch.full((nws // 8 + 1,), float('nan'), dtype=torch.float64, device=DEV)
    d_off, d_len = _dev(offs, torch.int64), _dev(lens, torch.int32)
    d_gm, d_gs = (None, None) if gmean is None else (_dev(gmean), _dev(gstd))
    d_noise = None if noise is None else _dev(noise, torch.float32)
    d_ranges = None if ranges is None else _dev(np.asarray(ranges, np.int32).reshape(B, -1, 4))
    NR = 0 if ranges is None else d_ranges.shape[1]
    rc = lib.otr_feature_prepare(_p(src), _p(d_off), _p(d_len), B, Tmax, F, mode, _p(d_gm), _p(d_gs), _p(d_noise), _p(d_ranges), NR,
                                 _p(dst), _p(mask), _p(stats), _p(ws), nws, _stream())
    assert rc == 0, lib.otr_last_error_string()
    torch.cuda.synchronize()
    return (dst.reshape(B, Tmax, F).cpu().numpy(), None if mask is None else mask.cpu().numpy(),
            None if stats is None else stats.cpu().numpy())


def check(got, want, mode, what):
    dst, mask, stats = got
    assert not np.isnan(want['dst']).all()
    ok = np.ones(dst.shape[0], bool)
    if mode == 1:                                            # fewer than two values: NaN by IEEE on both sides, not compared
        ok = ~np.isnan(want['stats'][:, 1]) | ~want['mask'].any(1)
    assert not np.isnan(dst[ok]).any(), what                # every cell written
    err = np.abs(dst[ok] - want['dst'][ok])
    worst = float((err / np.maximum(want['bound'][ok], 1e-300)).max()) if (want['bound'][ok] > 0).any() else 0.0
    print('%s: worst error / bound %.3f' % (what, worst))
    assert np.all(err <= want['bound'][ok]), (what, worst)
    for b in np.nonzero(~ok)[0]:
        assert not dst[b][~want['mask'][b]].view(np.uint32).any(), what
    if mask is not None:
        assert np.array_equal(mask, want['mask'].astype(np.uint8)), what
    if mode == 1 and stats is not None:
        live = ok & want['mask'].any(1)
        rel = np.abs(stats[live] - want['stats'][live]) / np.abs(want['stats'][live])
        print('%s: worst stats error %.3f x 2^-23' % (what, float(rel.max()) / ref.EPS32))
        assert np.all(rel <= ref.EPS32), (what, rel.max())


@pytest.mark.parametrize('form', ['packed', 'inplace'])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('F', [1, 3, 40, 80, 83])
def test_parity_with_the_float64_restatement(F, mode, form):
    """every batch size; spans starting on 4-, 8- and 16-byte boundaries (odd F: by the frame gaps 0..3; even F: by shifting the
    buffer one and two floats), dst rows likewise"""
    for B in (1, 3, 33):
        utts, gmean, gstd = _batch(B, F)
        want = _want(B, F, mode)
        for shift in (0, 1, 2):
            got = run_entry(utts, max(BATCHES[B]), mode, form, gmean, gstd, src_shift=shift, dst_shift=(shift * 3) % 4)
            check(got, want, mode, 'F=%d mode=%d %s B=%d shift=%d' % (F, mode, form, B, shift))


def test_copy_mode_is_exact():
    utts, _, _ = _batch(3, 83)
    dst, mask, stats = run_entry(utts, 1401, 0)
    want = _want(3, 83, 0)
    assert np.array_equal(dst.astype(np.float64), want['dst']) and np.array_equal(mask, want['mask'].astype(np.uint8))
    assert np.isnan(stats).all()                             # stats belong to mode 1


@pytest.mark.parametrize('T,F', [(65, 40), (1000, 80)])
@pytest.mark.parametrize('form', ['packed', 'inplace'])
def test_large_offset_data(T, F, form):
    """mean 1000, std 0.1: a single-pass fp32 sum of squares fails this bound by > 1000x or gives NaN"""
    rng = np.random.default_rng(T)
    utts = [(1000.0 + 0.1 * rng.standard_normal((T, F))).astype(np.float32)]
    want = ref.prepare(utts, T, 'utterance')
    assert 5000 < abs(want['stats'][0, 0]) / want['stats'][0, 1] < 20000
    check(run_entry(utts, T, 1, form), want, 1, 'large offset %dx%d %s' % (T, F, form))


def _ordered_case():
    rng = np.random.default_rng(77)
    F, lens = 83, [257, 64, 300]
    utts = [(rng.standard_normal((T, F)) * 2 + 3).astype(np.float32) for T in lens]
    noise = (rng.standard_normal((3, F)) * 0.5).astype(np.float32)
    ranges = [[(0, 257, 10, 19), (250, 257, 0, 83), (3, 40, 80, 83), (100, 120, 0, 83)],       # touching t = len and f = F
              [(0, 64, 0, 1), (63, 64, 0, 83), (10, 20, 82, 83), (0, 1, 0, 83)],
              [(0, 300, 40, 44), (299, 300, 0, 83), (5, 6, 70, 83), (290, 310, 5, 9)]]       # the last one runs past the utterance
    return utts, noise, ranges


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_noise_then_rectangles_and_exact_zeros(mode):
    utts, noise, ranges = _ordered_case()
    gmean, gstd = np.full(83, 3.0, np.float32), np.full(83, 2.0, np.float32)
    Tmax = 320
    want = ref.prepare(utts, Tmax, MODES[mode], gmean, gstd, noise, ranges)
    got = run_entry(utts, Tmax, mode, 'packed', gmean, gstd, noise, ranges)
    check(got, want, mode, 'ordered mode=%d' % mode)
    zero = ref.zero_cells([257, 64, 300], Tmax, 83, ranges)
    assert zero[0, 250:257].all() and zero[0, 3:40, 80:].all() and zero[2, 290:300, 5:9].all() and not zero[0, 0, 0]
    assert not got[0][zero].view(np.uint32).any()            # +0.0 bit for bit, noise or not
    assert (got[0][~zero] != 0).all()                        # and nothing else was zeroed
    # the same through the in-place form, and with empty rectangles added: the same bits
    again = run_entry(utts, Tmax, mode, 'inplace', gmean, gstd, noise, ranges)
    assert np.array_equal(again[0].view(np.uint32), got[0].view(np.uint32))
    empty = [r + [(5, 5, 0, 83), (0, 400, 7, 7), (9, 3, 0, 83), (0, 400, 50, 20)] for r in ranges]
    more = run_entry(utts, Tmax, mode, 'packed', gmean, gstd, noise, empty)
    assert np.array_equal(more[0].view(np.uint32), got[0].view(np.uint32))
    # noise alone (no rectangles) only differs inside the rectangles
    plain = run_entry(utts, Tmax, mode, 'packed', gmean, gstd, noise, None)
    assert np.array_equal(plain[0][~zero].view(np.uint32), got[0][~zero].view(np.uint32))


def test_mask_clamped_lengths_and_an_empty_utterance():
    rng = np.random.default_rng(5)
    F, Tmax = 40, 70
    utts = [(rng.standard_normal((T, F)) + 1).astype(np.float32) for T in (70, 33, 70)]
    base = run_entry(utts, Tmax, 1)
    want = ref.prepare(utts, Tmax, 'utterance')
    check(base, want, 1, 'base')
    assert np.array_equal(base[1].astype(bool), np.arange(Tmax)[None, :] < np.array([70, 33, 70])[:, None])
    # lengths above Tmax are clamped: the same bits
    clamped = run_entry(utts, Tmax, 1, lengths=[75, 33, 1 << 30])
    for a, b in zip(base, clamped):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # an empty utterance in the middle, and a negative length, leave the others alone
    withempty = [utts[0], np.zeros((0, F), np.float32), utts[1], utts[2]]
    for form in ('packed', 'inplace'):
        dst, mask, stats = run_entry(withempty, Tmax, 1, form, lengths=[70, 0 if form == 'packed' else -4, 33, 70])
        keep = [0, 2, 3]
        assert np.array_equal(dst[keep].view(np.uint32), base[0].view(np.uint32)) and np.array_equal(mask[keep], base[1])
        assert np.array_equal(stats[keep].view(np.uint32), base[2].view(np.uint32))
        assert not dst[1].view(np.uint32).any() and not mask[1].any()
    # optional outputs may be left out
    dst, mask, stats = run_entry(utts, Tmax, 1, want_mask=False, want_stats=False)
    assert mask is None and stats is None and np.array_equal(dst.view(np.uint32), base[0].view(np.uint32))


def test_same_call_same_bits():
    utts, _, _ = _batch(33, 83)
    a = run_entry(utts, 1401, 1)
    b = run_entry(utts, 1401, 1)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def _ragged_calls():
    rng = np.random.default_rng(11)
    F = 83
    calls = []
    for lens in ([1, 64, 300], [257, 2, 0, 65, 1000], [63]):
        utts = [(rng.standard_normal((T, F)) * 3 + 5 + 0.1 * np.arange(F)).astype(np.float32) for T in lens]
        offs, cur = [], 0
        for u in utts:
            cur += 1
            offs.append(cur)
            cur += u.shape[0]
        host = np.full((cur + 1, F), np.nan, np.float32)
        for o, u in zip(offs, utts):
            host[o:o + u.shape[0]] = u
        calls.append((utts, _dev(host), _dev(offs, torch.int64), _dev(lens, torch.int32)))
    return F, calls


def test_cmvn_accumulate_against_numpy_and_repeatable():
    F, calls = _ragged_calls()
    want = sum(ref.cmvn_sums(c[0]) for c in calls)
    runs = []
    for _ in range(2):
        acc = torch.zeros(2 * F + 1, dtype=torch.float64, device=DEV)
        for _, src, off, ln in calls:
            assert ops.cmvn_accumulate(src, off, ln, acc) is acc
        runs.append(acc.cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    assert runs[0][2 * F] == want[2 * F] == 1 + 64 + 300 + 257 + 2 + 65 + 1000 + 63
    rel = np.abs(runs[0][:2 * F] - want[:2 * F]) / np.abs(want[:2 * F])
    print('cmvn sums: worst relative error %.2e' % rel.max())
    assert rel.max() <= 1e-10
    cm = data.GlobalCMVN(F, DEV)
    for _, src, off, ln in calls:
        cm.update(src, off, ln)
    allx = np.concatenate([u for c in calls for u in c[0]]).astype(np.float64)
    mean, std = cm.result()
    np.testing.assert_allclose(mean.numpy(), allx.mean(0), rtol=1e-6)
    np.testing.assert_allclose(std.numpy(), allx.std(0), rtol=1e-6)
    # the padded form gives the same statistics
    cp = data.GlobalCMVN(F, DEV)
    for utts, _, _, _ in calls:
        Tm = max(u.shape[0] for u in utts)
        pad = np.full((len(utts), Tm, F), np.nan, np.float32)
        for b, u in enumerate(utts):
            pad[b, :u.shape[0]] = u
        cp.update_padded(_dev(pad), _dev([u.shape[0] for u in utts], torch.int32))
    np.testing.assert_allclose(cp.acc.cpu().numpy(), want, rtol=1e-10)


def test_wrapper_matches_the_entry():
    utts, gmean, gstd = _batch(3, 83)
    want = _want(3, 83, 1)
    lens = [u.shape[0] for u in utts]
    src = _dev(np.concatenate(utts))
    off = _dev(np.concatenate(([0], np.cumsum(lens[:-1]))), torch.int64)
    feats, mask, stats = ops.feature_prepare(src, off, _dev(lens, torch.int32), 1401, norm='utterance', want_stats=True)
    assert mask.dtype == torch.bool and feats.shape == (3, 1401, 83)
    check((feats.cpu().numpy(), mask.cpu().numpy().astype(np.uint8), stats.cpu().numpy()), want, 1, 'ops.feature_prepare')
    out = torch.full((3, 1401, 83), float('nan'), device=DEV)
    f2, m2 = ops.feature_prepare(src, off, _dev(lens, torch.int32), 1401, norm='global', gmean=_dev(gmean), gstd=_dev(gstd), out=out)
    assert f2.data_ptr() == out.data_ptr()
    check((f2.cpu().numpy(), m2.cpu().numpy().astype(np.uint8), None), _want(3, 83, 2), 2, 'ops.feature_prepare global')
    with pytest.raises(_lib.OtransHipError):
        ops.feature_prepare(src.cpu(), off, _dev(lens, torch.int32), 1401)
    with pytest.raises(_lib.OtransHipError):
        ops.cmvn_accumulate(src, off.cpu(), _dev(lens, torch.int32), torch.zeros(167, dtype=torch.float64, device=DEV))


SPEC = dict(freq_mask_num=2, time_mask_num=3, freq_mask_rate=0.3, time_mask_rate=0.05)


def _raw_batch():
    rng = np.random.default_rng(21)
    out = []
    for i, (T, Lt) in enumerate([(257, 4), (1000, 7), (64, 1), (300, 5)]):
        feat = torch.from_numpy((rng.standard_normal((T, 80)) * 2 + 4).astype(np.float32))
        out.append(('utt%d' % i, feat, T, [int(v) for v in rng.integers(3, 50, Lt)], Lt))
    return out


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def test_pipeline_agrees_with_the_existing_pieces():
    """FeaturePipeline on raw features against collate_fn_with_eos_bos on features normalised with CPU torch.std_mean plus the same
    noise, followed by spec_augment_batch, all under the same seeds"""
    batch = _raw_batch()
    sigma = 0.3
    pipe = data.FeaturePipeline(dict(normalization=True, gaussian_noise=sigma, spec_augment=True, spec_augment_config=SPEC))
    _seed(3)
    ids, inputs, targets = pipe(batch, DEV)
    _seed(3)
    composed, scale = [], []
    for utt, feat, T, tgt, Lt in batch:
        std, mean = torch.std_mean(feat)
        composed.append((utt, (feat - mean) / std + torch.normal(torch.zeros(80), std=sigma), T, tgt, Lt))
        scale.append(abs(float(mean)) / float(std))
    ids2, in2, tg2 = data.collate_fn_with_eos_bos(composed, DEV)
    data.spec_augment_batch(in2['inputs'], in2['inputs_length'].tolist(), **SPEC)
    assert ids == ids2
    a, b = inputs['inputs'].cpu().numpy(), in2['inputs'].cpu().numpy().astype(np.float64)
    assert np.array_equal(a == 0, b == 0) and (b[0, :257] == 0).any()
    bound = 2 * ref.EPS32 * (np.abs(b) + np.asarray(scale)[:, None, None] + 1)
    print('pipeline against the composed path: worst error / bound %.3f' % float((np.abs(a - b) / bound).max()))
    assert np.all(np.abs(a - b) <= bound)
    assert inputs['mask'].dtype == in2['mask'].dtype and torch.equal(inputs['mask'], in2['mask'])
    assert inputs['inputs_length'].dtype == in2['inputs_length'].dtype and torch.equal(inputs['inputs_length'], in2['inputs_length'])
    for k in tg2:
        assert targets[k].dtype == tg2[k].dtype and torch.equal(targets[k], tg2[k]), k
    # evaluation: normalisation only -- no noise, no masking
    ev = data.FeaturePipeline(dict(normalization=True, gaussian_noise=sigma, spec_augment=True, spec_augment_config=SPEC), is_eval=True)
    _, in3, _ = ev(batch, DEV)
    c = in3['inputs'].cpu().numpy()
    for i, (_, feat, T, _, _) in enumerate(batch):
        y = ref.chain(feat.numpy(), 'utterance')
        assert (c[i, :T] != 0).all() and not c[i, T:].any()
        assert np.all(np.abs(c[i, :T] - y) <= 2 * ref.EPS32 * (np.abs(y) + scale[i] + 1))


def test_pipeline_with_global_cmvn_files(tmp_path):
    batch = _raw_batch()
    cm = data.GlobalCMVN(80, DEV)
    _, raw, _ = data.collate_fn_with_eos_bos(batch, DEV)
    cm.update_padded(raw['inputs'], raw['inputs_length'])
    cm.save(str(tmp_path / 'cmvn'))
    pipe = data.FeaturePipeline(dict(normalization=True, global_cmvn=str(tmp_path / 'cmvn'), spec_augment=False))
    _, inputs, _ = pipe(batch, DEV)
    gmean, gstd = data.GlobalCMVN.load(str(tmp_path / 'cmvn'))
    want = ref.prepare([d[1].numpy() for d in batch], 1000, 'global', gmean.numpy(), gstd.numpy())
    check((inputs['inputs'].cpu().numpy(), inputs['mask'].cpu().numpy().astype(np.uint8), None), want, 2, 'pipeline global cmvn')


def test_compute_cmvn_tool_writes_the_two_files(tmp_path):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location('compute_cmvn', Path(__file__).resolve().parent.parent / 'tools' / 'compute_cmvn.py')
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(4)
    utts = [(rng.standard_normal((T, 40)) * 2 + np.arange(40)).astype(np.float32) for T in (30, 1, 257, 64, 100)]
    paths = []
    for i, u in enumerate(utts):
        paths.append(str(tmp_path / ('u%d.npy' % i)))
        np.save(paths[-1], u)
    np.savez(str(tmp_path / 'all.npz'), **{'u%d' % i: u for i, u in enumerate(utts)})
    allx = np.concatenate(utts).astype(np.float64)
    for inputs, prefix in ((paths, 'a'), ([str(tmp_path / 'all.npz')], 'b')):
        cm = tool.compute(inputs, 2, DEV)                     # batches of 2, 2 and 1 utterances
        cm.save(str(tmp_path / prefix))
        mean, std = data.GlobalCMVN.load(str(tmp_path / prefix))
        assert float(cm.acc[80]) == 452
        np.testing.assert_allclose(mean.numpy(), allx.mean(0), rtol=1e-6)
        np.testing.assert_allclose(std.numpy(), allx.std(0), rtol=1e-6)


def test_refusals_leave_device_outputs_alone():
    lib = _lib.load()
    B, Tmax, F = 2, 5, 4
    src = torch.arange(B * Tmax * F, dtype=torch.float32, device=DEV) / 7
    off, ln = _dev([0, 5], torch.int64), _dev([5, 3], torch.int32)
    vec = torch.ones(F, device=DEV)
    noise, ranges = torch.zeros(B, F, device=DEV), torch.zeros(B, 2, 4, dtype=torch.int32, device=DEV)
    dst = torch.full((B, Tmax, F), float('nan'), device=DEV)
    mask = torch.full((B, Tmax), 0xFF, dtype=torch.uint8, device=DEV)
    stats = torch.full((B, 2), float('nan'), device=DEV)
    ws = torch.full((16,), float('nan'), dtype=torch.float64, device=DEV)
    nws = lib.otr_feature_prepare_workspace_bytes(B, Tmax, F)
    assert nws == 48

    def call(src=src, off=off, ln=ln, B=B, Tmax=Tmax, F=F, mode=1, gmean=vec, gstd=vec, noise=noise, ranges=ranges, NR=2, dst=dst,
             ws=ws, nws=nws):
        return lib.otr_feature_prepare(_p(src), _p(off), _p(ln), B, Tmax, F, mode, _p(gmean), _p(gstd), _p(noise), _p(ranges), NR,
                                       _p(dst), _p(mask), _p(stats), _p(ws), nws, _stream())
    bad = [dict(src=None), dict(off=None), dict(ln=None), dict(dst=None), dict(B=-1), dict(Tmax=0), dict(F=0), dict(NR=-1), dict(NR=65),
           dict(NR=1, ranges=None), dict(mode=-1), dict(mode=3), dict(mode=2, gmean=None), dict(mode=2, gstd=None), dict(nws=nws - 1),
           dict(ws=None)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert b'feature_prepare' in lib.otr_last_error_string()
    torch.cuda.synchronize()
    assert torch.isnan(dst).all() and (mask == 0xFF).all() and torch.isnan(stats).all() and torch.isnan(ws).all()
    for shape in ((-1, 5, 4), (2, 0, 4), (2, 5, 0), (65536, 5, 4), (2, 1 << 20, 1 << 11)):
        assert lib.otr_feature_prepare_workspace_bytes(*shape) == -1, shape
    assert call() == 0                                       # and the accepted call writes every output
    torch.cuda.synchronize()
    assert not torch.isnan(dst).any() and mask.cpu().tolist() == [[1] * 5, [1, 1, 1, 0, 0]] and not torch.isnan(stats).any()
