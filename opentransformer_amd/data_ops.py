"""No-autograd wrappers over the C ABI (include/otrans_hip.h) for what builds batches and language models from data: feature
preparation, the MixSpeech mix and the n-gram estimator's passes.  The rules are those of ops.py: raw data_ptr()s and torch's current
stream go to libotrans_hip.so, a non-CUDA tensor raises.  ops.py re-exports every public name below; callers write `ops.X`."""
import ctypes as C

import torch

from . import _lib as L
from ._runtime import _cuda, _p, _stream, _timed, _len32

__all__ = ['feature_prepare', 'cmvn_accumulate', 'FEATPREP_MAX_RANGES', 'mixspeech_mix', 'ngram_train_count', 'ngram_train_stats',
           'ngram_train_estimate', 'NGRAM_TRAIN_ERRORS']

NGRAM_TRAIN_ERRORS = {1: 'the count table is full', 2: 'an id inside a sentence is outside [1, V) or is the </s> unit',
                      4: 'a sentence length is outside [0, L]', 8: 'a context or a suffix is missing from the count table'}


def ngram_train_count(tokens, lengths, order, V, eos, table_capacity):
    """The count pass of the n-gram estimator (include/otrans_hip.h otr_ngram_count).  tokens int64 [n, L] on a GPU, rows strided
    freely, lengths int32 [n]; nothing at or beyond a length is read.  Returns (table int64 [table_capacity, 4]: the count entries
    { key, raw | cont << 32, sum | n1 << 32, n2 | n3p << 32 }, err int32 [1]: the error bits, to be read by the caller)."""
    _cuda(tokens, lengths)
    if tokens.dtype != torch.int64 or tokens.dim() != 2 or lengths.dtype != torch.int32 or lengths.shape != tokens.shape[:1]:
        raise L.OtransHipError('ngram_train_count: tokens int64 [n, L] and lengths int32 [n] expected, got %s %s %s %s'
                               % (tokens.dtype, tuple(tokens.shape), lengths.dtype, tuple(lengths.shape)))
    n, T = tokens.shape
    if T and tokens.stride(1) != 1:
        tokens = tokens.contiguous()
    dev = tokens.device
    table = torch.zeros((int(table_capacity), 4), dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.load().otr_ngram_count(_p(tokens) if n and T else None, tokens.stride(0) if n > 1 and T else T, _p(lengths.contiguous()), n, T,
                                     int(order), int(V), int(eos), _p(table), int(table_capacity), _p(err), _stream()), 'otr_ngram_count')
    return table, err


def ngram_train_stats(table, order, V, err):
    """The statistics pass (otr_ngram_stats): fills the context statistics of `table` in place; returns glob int64 [20] on the device:
    sum, n1, n2, n3p of the empty context, then the count-of-counts nn[m][k] at 4 + 4 (m-1) + (k-1)."""
    _cuda(table, err)
    glob = torch.zeros(20, dtype=torch.int64, device=table.device)
    L.check(L.load().otr_ngram_stats(_p(table), table.shape[0], int(order), int(V), _p(glob), _p(err), _stream()), 'otr_ngram_stats')
    return glob


def ngram_train_estimate(table, order, V, n_units, discounts, glob, err):
    """The probability passes (otr_ngram_estimate, one launch per order): discounts [order][3] host floats.  Returns (logp f32,
    backoff f32) per count entry; the entries of empty slots are not written."""
    _cuda(table, glob, err)
    cap, dev = table.shape[0], table.device
    prob = torch.empty(cap, dtype=torch.float64, device=dev)
    logp = torch.empty(cap, dtype=torch.float32, device=dev)
    backoff = torch.empty(cap, dtype=torch.float32, device=dev)
    d = (C.c_double * (3 * int(order)))(*[float(v) for row in discounts for v in row])
    L.check(L.load().otr_ngram_estimate(_p(table), cap, int(order), int(V), int(n_units), d, _p(glob), _p(prob), _p(logp), _p(backoff),
                                        _p(err), _stream()), 'otr_ngram_estimate')
    return logp, backoff


# ------------------------------------------------------------------ feature preparation for batch assembly (csrc/featprep.hip)
FEATPREP_MAX_RANGES = 64
_FEATPREP_MODES = {None: 0, 'utterance': 1, 'global': 2}


def _ragged_index(src, row_off, lengths, what):
    """(src, row_off int64 [B], lengths int32 [B], B, F) of a packed ragged [.., F] float32 device buffer, as the entries take them"""
    _cuda(src, row_off, lengths)
    if src.dtype != torch.float32 or src.dim() < 2 or not src.is_contiguous():
        raise L.OtransHipError('%s: src must be a contiguous float32 [.., F] tensor, got %s %s' % (what, src.dtype, tuple(src.shape)))
    ro, ln = row_off.to(torch.int64).contiguous(), lengths.to(torch.int32).contiguous()
    if ro.dim() != 1 or ln.shape != ro.shape:
        raise L.OtransHipError('%s: row_off and lengths must both be [B], got %s and %s' % (what, tuple(row_off.shape), tuple(lengths.shape)))
    return src, ro, ln, ro.shape[0], src.shape[-1]


def feature_prepare(src, row_off, lengths, Tmax, norm=None, gmean=None, gstd=None, noise=None, ranges=None, out=None, want_stats=False):
    """The reference's post-fbank chain (normalisation -> gaussian noise -> SpecAugment, otrans/data/audio.py:125-136) and the zero
    padding of the collate in one call (include/otrans_hip.h otr_feature_prepare).  src float32 [sum T, F] holds utterance b as the
    rows row_off[b] .. row_off[b] + lengths[b] (device tensors [B]; lengths above Tmax are clamped); norm None | 'utterance' (scalar
    mean and unbiased std per utterance) | 'global' ((x - gmean[F]) / gstd[F]); noise float32 [B, F] is added to every frame of its
    utterance; ranges int32 [B, NR, 4] = {t0, t1, f0, f1} are zeroed last.  out: a float32 [B, Tmax, F] buffer to fill (src itself
    with row_off = arange(B) * Tmax is the in-place form).  Returns (feats [B, Tmax, F], mask bool [B, Tmax][, stats f32 [B, 2] = the
    mean and std of 'utterance']).  At most two launches on the current stream, no host synchronisation, bit-identical run to run."""
    if norm not in _FEATPREP_MODES:
        raise ValueError("feature_prepare: norm must be None, 'utterance' or 'global', got %r" % (norm,))
    if norm == 'global' and (gmean is None or gstd is None):
        raise ValueError("feature_prepare: norm='global' needs gmean and gstd")
    src, ro, ln, B, F_ = _ragged_index(src, row_off, lengths, 'feature_prepare')
    _cuda(gmean, gstd, noise, ranges, out)
    Tmax, dev = int(Tmax), src.device
    if norm == 'global':
        gmean, gstd = gmean.to(torch.float32).contiguous(), gstd.to(torch.float32).contiguous()
        if gmean.shape != (F_,) or gstd.shape != (F_,):
            raise L.OtransHipError('feature_prepare: gmean / gstd must be [%d], got %s and %s' % (F_, tuple(gmean.shape), tuple(gstd.shape)))
    else:
        gmean = gstd = None
    if noise is not None:
        noise = noise.to(torch.float32).contiguous()
        if noise.shape != (B, F_):
            raise L.OtransHipError('feature_prepare: noise must be [%d, %d], got %s' % (B, F_, tuple(noise.shape)))
    NR = 0
    if ranges is not None:
        ranges = ranges.to(torch.int32).contiguous()
        if ranges.dim() != 3 or ranges.shape[0] != B or ranges.shape[2] != 4 or ranges.shape[1] > FEATPREP_MAX_RANGES:
            raise L.OtransHipError('feature_prepare: ranges must be [%d, NR <= %d, 4], got %s' % (B, FEATPREP_MAX_RANGES, tuple(ranges.shape)))
        NR = ranges.shape[1]
        if NR == 0:
            ranges = None
    if out is None:
        out = torch.empty((B, Tmax, F_), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != B * Tmax * F_ or not out.is_contiguous():
        raise L.OtransHipError('feature_prepare: out must be a contiguous float32 buffer of %d x %d x %d values' % (B, Tmax, F_))
    lib = L.load()
    nws = lib.otr_feature_prepare_workspace_bytes(B, Tmax, F_)
    if nws < 0:
        raise L.OtransHipError('feature_prepare: shape B=%d Tmax=%d F=%d is not supported' % (B, Tmax, F_))
    ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=dev)
    mask = torch.empty((B, Tmax), dtype=torch.bool, device=dev)
    stats = torch.empty((B, 2), dtype=torch.float32, device=dev) if want_stats else None
    L.check(_timed('feature_prepare %dx%dx%d' % (B, Tmax, F_), {'bytes': (src.numel() + B * Tmax * F_) * 4},
                   lambda: lib.otr_feature_prepare(_p(src), _p(ro), _p(ln), B, Tmax, F_, _FEATPREP_MODES[norm], _p(gmean), _p(gstd),
                                                   _p(noise), _p(ranges), NR, _p(out), _p(mask), _p(stats), _p(ws), nws, _stream())),
            'otr_feature_prepare')
    out = out.view(B, Tmax, F_)
    return (out, mask, stats) if want_stats else (out, mask)


def cmvn_accumulate(src, row_off, lengths, acc):
    """Add to acc float64 [2F + 1] the per-dimension sums, sums of squares and the frame count of the live frames of a packed ragged
    batch (src / row_off / lengths as feature_prepare takes them; include/otrans_hip.h otr_cmvn_accumulate).  One launch, fixed
    summation order.  Returns acc."""
    src, ro, ln, B, F_ = _ragged_index(src, row_off, lengths, 'cmvn_accumulate')
    _cuda(acc)
    if acc.dtype != torch.float64 or acc.shape != (2 * F_ + 1,) or not acc.is_contiguous():
        raise L.OtransHipError('cmvn_accumulate: acc must be a contiguous float64 [%d] tensor' % (2 * F_ + 1))
    L.check(L.load().otr_cmvn_accumulate(_p(src), _p(ro), _p(ln), B, F_, _p(acc), _stream()), 'otr_cmvn_accumulate')
    return acc


# ------------------------------------------------------------------ MixSpeech: the mixed half batch (csrc/mixspeech.hip)
def _lam_check(who, lam):
    """the mixing weight of MixSpeech as mixspeech_mix and loss_ops.ctc_loss_pair take it"""
    if not torch.is_tensor(lam) or lam.numel() != 1:
        raise ValueError('%s: lam must be a 1-element device tensor, got %r' % (who, lam if not torch.is_tensor(lam) else tuple(lam.shape)))


def mixspeech_mix(x, lengths, lam):
    """The mixed half batch of MixSpeech (include/otrans_hip.h otr_mixspeech_mix): x f32 [B, T, F] (unit stride over T and F; the
    utterance pitch is passed on), lengths [B] (int32 or int64), lam a 1-element f32 DEVICE tensor.  Returns (out f32 [P, T, F],
    out_lengths int32 [P], out_mask bool [P, T]) with P = B // 2: out[p] = lam * x[2p] + (1 - lam) * x[2p + 1] bit for bit as float32
    torch forms it on zero-padded input, with the length and mask of the longer utterance.  Frames at or past an utterance's length are
    not read.  One launch, no host synchronisation, no gradient (the features are data)."""
    who = 'mixspeech_mix'
    if x.dim() != 3:
        raise ValueError('%s: x must be [B, T, F], got %s' % (who, tuple(x.shape)))
    B, T, F_ = x.shape
    if B < 2 or T < 1 or F_ < 1:
        raise ValueError('%s: x [B, T, F] = %s needs B >= 2, T >= 1 and F >= 1' % (who, (B, T, F_)))
    if lengths.numel() != B:
        raise ValueError('%s: lengths must hold B = %d entries, got %s' % (who, B, tuple(lengths.shape)))
    _lam_check(who, lam)
    _cuda(x, lengths, lam)
    if x.dtype != torch.float32 or lam.dtype != torch.float32 or lengths.dtype not in (torch.int32, torch.int64):
        raise L.OtransHipError('%s: x f32, lengths int32 (or int64), lam f32 expected' % who)
    x = x.detach()
    if not (x.stride(2) == 1 and x.stride(1) == F_ and x.stride(0) >= T * F_):
        x = x.contiguous()
    P = B // 2
    out = torch.empty((P, T, F_), dtype=torch.float32, device=x.device)
    out_len = torch.empty((P,), dtype=torch.int32, device=x.device)
    out_mask = torch.empty((P, T), dtype=torch.bool, device=x.device)
    L.check(L.load().otr_mixspeech_mix(_p(x), x.stride(0), _p(_len32(lengths)), _p(lam), B, T, F_, _p(out), _p(out_len), _p(out_mask),
                                       _stream()), 'otr_mixspeech_mix')
    return out, out_len, out_mask
