"""Batch assembly for the hot path: the reference's collate + SpecAugment, with the padded batch
built directly in device memory.

* `collate_fn_with_eos_bos(batch, device)`: otrans/data/loader.py:66-108 -- pad features with zeros, bool masks,
  targets `[BOS] tokens [EOS] PAD*`, `targets_length` counting the EOS.  Features may already live on the device (they are
  copied into ONE preallocated [B,Tmax,F] buffer; no per-utterance F.pad + cat).
* `BySequenceLengthSampler`: otrans/data/bucket.py:14-170 -- length-bucketed batches (same batches as the reference under
  the same `random` seed), which bound the padding of those device batches.
* `spec_augment_ranges` + `spec_augment_batch`: otrans/data/augment.py:9-41.  The mask rectangles are drawn on the host
  with the reference's exact sequence of `np.random.uniform` / `random.randint` calls (so a seeded run produces the same
  masks), then applied to the whole batch by one kernel (otr_spec_mask) instead of per-utterance numpy slicing.
* `FeaturePipeline`: otrans/data/audio.py:125-136 + the collate -- the whole per-utterance chain after the fbank (normalisation or
  global CMVN -> gaussian noise -> SpecAugment) from RAW features: one upload of the concatenated utterances, one
  otr_feature_prepare call that normalises, adds the noise, masks and pads.  `GlobalCMVN` accumulates the sums behind the
  `<prefix>.mean.npy` / `<prefix>.std.npy` files audio.py:44-45 loads (tools/compute_cmvn.py writes them).
"""
import ctypes as C
import random

import numpy as np
import torch
import torch.utils.data

from . import _lib as L
from . import ops

PAD, BOS, EOS = 0, 1, 1          # otrans/data/__init__.py:7-12


def collate_fn_with_eos_bos(batch, device=None):
    """batch: list of (utt_id, feat [T_i, F] float tensor, feat_len, target (list of ints), target_len)."""
    utt_ids = [d[0] for d in batch]
    features_length = [int(d[2]) for d in batch]
    Tmax = max(features_length)
    device = torch.device(device) if device is not None else batch[0][1].device
    F_ = batch[0][1].shape[-1]
    feats = torch.zeros((len(batch), Tmax, F_), dtype=torch.float32, device=device)
    for i, (_, feat, flen, _, _) in enumerate(batch):
        feats[i, :flen].copy_(feat[:flen], non_blocking=True)
    flen_t = torch.tensor(features_length, dtype=torch.int32)
    fmask = torch.arange(Tmax).unsqueeze(0) < flen_t.unsqueeze(1)
    inputs = {'inputs': feats, 'inputs_length': flen_t.to(device), 'mask': fmask.to(device)}
    return utt_ids, inputs, _targets_with_eos_bos(batch, device)


def _targets_with_eos_bos(batch, device):
    """the targets dict of the collate: `[BOS] tokens [EOS] PAD*`, `targets_length` counting the EOS"""
    targets_length = [int(d[4]) for d in batch]
    Lmax = max(targets_length)
    tg = torch.full((len(batch), Lmax + 2), PAD, dtype=torch.long)
    for i, (_, _, _, target, tlen) in enumerate(batch):
        tg[i, 0] = BOS
        tg[i, 1:1 + tlen] = torch.as_tensor(list(target)[:tlen], dtype=torch.long)
        tg[i, 1 + tlen] = EOS
    tlen_t = torch.tensor(targets_length, dtype=torch.int32)
    tmask = torch.arange(Lmax + 2).unsqueeze(0) < (tlen_t + 2).unsqueeze(1)
    return {'targets': tg.to(device), 'targets_length': (tlen_t + 1).to(device), 'mask': tmask.to(device)}


def spec_augment_ranges(tau, v, freq_mask_num=2, time_mask_num=2, freq_mask_rate=0.3, time_mask_rate=0.05,
                        max_mask_time_len=100):
    """The rectangles data/augment.py:9-41 would zero for a [tau, v] spectrogram, as rows {t0, t1, f0, f1}; consumes
    numpy's and `random`'s global generators in exactly the reference's order."""
    freq_para = int(v * freq_mask_rate)
    time_para = min(int(tau * time_mask_rate), max_mask_time_len)
    out = []
    for _ in range(freq_mask_num):
        f = int(np.random.uniform(low=0.0, high=freq_para))
        f0 = random.randint(0, v - f)
        out.append((0, tau, f0, f0 + f))
    for _ in range(time_mask_num):
        t = int(np.random.uniform(low=0.0, high=time_para))
        t0 = random.randint(0, tau - t)
        out.append((t0, t0 + t, 0, v))
    return out


def spec_augment_batch(inputs, lengths=None, **kw):
    """In-place SpecAugment of a padded device batch [B,T,F]: utterance b is treated as a [lengths[b], F] spectrogram
    (the reference augments each utterance before padding)."""
    if not inputs.is_cuda:
        raise L.OtransHipError('spec_augment_batch needs a CUDA/HIP tensor; there is no CPU fallback')
    B, T, F_ = inputs.shape
    lengths = [T] * B if lengths is None else [int(x) for x in lengths]
    rows = [spec_augment_ranges(lengths[b], F_, **kw) for b in range(B)]
    NR = len(rows[0])
    if NR == 0:
        return inputs
    r = torch.tensor(rows, dtype=torch.int32).reshape(B, NR, 4).to(inputs.device)
    x = inputs if inputs.is_contiguous() else inputs.contiguous()
    L.check(L.load().otr_spec_mask(C.c_void_p(x.data_ptr()), C.c_void_p(r.data_ptr()), B, NR, T, F_,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_spec_mask')
    if x is not inputs:
        inputs.copy_(x)
    return inputs


class FeaturePipeline:
    """What the reference's AudioDataset.__getitem__ does to an utterance after the fbank (otrans/data/audio.py:125-136) plus the
    collate, as one DataLoader `collate_fn` over RAW features.  `params` is the yaml's data section: `normalization` (with the optional
    `global_cmvn` file prefix: (x - mean[F]) / std[F] from `<prefix>.mean.npy` / `<prefix>.std.npy`, else the utterance's scalar
    torch.std_mean), `gaussian_noise` (std of ONE [F] vector per utterance, added to every frame: the reference's quirk),
    `spec_augment` + `spec_augment_config`.  Noise and SpecAugment are off when `is_eval`, normalisation stays on (audio.py:33,56-61).

    Random draws happen on the host per utterance in batch order -- torch.normal(zeros(F), std=sigma) when sigma > 0, then
    spec_augment_ranges -- the reference's order on its generators, so a seeded single-process run draws what the reference draws.
    Per batch: the features are concatenated once and uploaded once, offsets / lengths / rectangles ride in one small upload and the
    noise in another, and one otr_feature_prepare call writes the padded batch and its mask."""

    def __init__(self, params, is_eval=False):
        self.is_eval = is_eval
        self.norm, self.gmean, self.gstd = None, None, None
        if params['normalization']:
            self.norm = 'utterance'
            if 'global_cmvn' in params:
                self.norm = 'global'
                self.gmean, self.gstd = GlobalCMVN.load(params['global_cmvn'])
        self.gaussian_noise = float(params.get('gaussian_noise', 0.0)) if not is_eval else 0.0
        self.spec_augment = bool(params['spec_augment']) and not is_eval
        self.spec_augment_config = dict(params['spec_augment_config']) if self.spec_augment else {}
        self._cmvn_on = {}

    def draw(self, lengths, F_):
        """the batch's host-side draws: (noise float32 [B, F] or None, rectangles [B][NR] of (t0, t1, f0, f1) or None)"""
        noise, rows = [], []
        for length in lengths:
            if self.gaussian_noise > 0.0:
                noise.append(torch.normal(torch.zeros(F_), std=self.gaussian_noise))
            if self.spec_augment:
                rows.append(spec_augment_ranges(length, F_, **self.spec_augment_config))
        return (torch.stack(noise) if noise else None), (rows if rows and rows[0] else None)

    def __call__(self, batch, device=None):
        utt_ids = [d[0] for d in batch]
        lengths = [int(d[2]) for d in batch]
        if min(lengths) <= 0:
            raise ValueError('FeaturePipeline: utterance %r has no frames' % (utt_ids[lengths.index(min(lengths))],))
        device = torch.device(device) if device is not None else batch[0][1].device
        B, Tmax, F_ = len(batch), max(lengths), batch[0][1].shape[-1]
        noise, rows = self.draw(lengths, F_)
        src = torch.cat([d[1][:n].to(torch.float32) for d, n in zip(batch, lengths)]).to(device, non_blocking=True)
        # one int32 upload: row_off as int64 pairs [2B] | lengths [B] | rectangles [B, NR, 4]
        offs = np.concatenate(([0], np.cumsum(lengths[:-1]))).astype(np.int64)
        parts = [offs.view(np.int32), np.asarray(lengths, np.int32)]
        if rows is not None:
            parts.append(np.asarray(rows, np.int32).reshape(-1))
        idx = torch.from_numpy(np.concatenate(parts)).to(device, non_blocking=True)
        ranges = idx[3 * B:].view(B, -1, 4) if rows is not None else None
        if self.norm == 'global' and device not in self._cmvn_on:
            self._cmvn_on[device] = (self.gmean.to(device), self.gstd.to(device))
        gmean, gstd = self._cmvn_on.get(device, (None, None))
        feats, mask = ops.feature_prepare(src, idx[:2 * B].view(torch.int64), idx[2 * B:3 * B], Tmax, norm=self.norm, gmean=gmean,
                                          gstd=gstd, noise=None if noise is None else noise.to(device, non_blocking=True), ranges=ranges)
        inputs = {'inputs': feats, 'inputs_length': idx[2 * B:3 * B], 'mask': mask}
        return utt_ids, inputs, _targets_with_eos_bos(batch, device)


class GlobalCMVN:
    """Per-dimension mean and std of a feature corpus, accumulated on the device in float64 (ops.cmvn_accumulate: sums, sums of squares
    and the frame count, in a fixed order).  result() forms them on the host with the POPULATION std, sqrt(max(E[x^2] - mean^2, 0)),
    Kaldi's convention (the reference loads the two files and defines no way to make them)."""

    def __init__(self, F_, device):
        self.F = int(F_)
        self.acc = torch.zeros(2 * self.F + 1, dtype=torch.float64, device=device)

    def update(self, src, row_off, lengths):
        """src float32 [sum T, F] with utterance b at rows row_off[b] .. row_off[b] + lengths[b] (device tensors)"""
        ops.cmvn_accumulate(src, row_off, lengths, self.acc)

    def update_padded(self, inputs, lengths):
        """a padded batch [B, T, F] with its lengths [B], e.g. the `inputs` / `inputs_length` of a collate over raw features"""
        B, T, _ = inputs.shape
        ops.cmvn_accumulate(inputs.contiguous(), torch.arange(B, dtype=torch.int64, device=inputs.device) * T, lengths, self.acc)

    def result(self):
        """(mean [F], std [F]) as float32 CPU tensors"""
        acc = self.acc.cpu().numpy()
        n = acc[2 * self.F]
        mean = acc[:self.F] / n
        std = np.sqrt(np.maximum(acc[self.F:2 * self.F] / n - mean * mean, 0.0))
        return torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(std.astype(np.float32))

    def save(self, prefix):
        mean, std = self.result()
        np.save(prefix + '.mean.npy', mean.numpy())
        np.save(prefix + '.std.npy', std.numpy())

    @staticmethod
    def load(prefix):
        """(mean [F], std [F]) float32 CPU tensors from `<prefix>.mean.npy` / `<prefix>.std.npy`"""
        return (torch.from_numpy(np.load(prefix + '.mean.npy').astype(np.float32)),
                torch.from_numpy(np.load(prefix + '.std.npy').astype(np.float32)))


class BySequenceLengthSampler(torch.utils.data.Sampler):
    """Length-bucketed batch sampler with the reference's semantics (otrans/data/bucket.py:14-170), so that a seeded
    `random` yields the very same batches: utterances go to the bucket whose (lower, upper] frame range holds them, each
    bucket is shuffled and cut into batches -- of `bucket_batch_size[min(id, last)]` utterances, or (the default,
    `audo_set_batch_size`, spelled as in the reference) greedily up to `max_frames_one_batch` frames -- and the batches of
    all buckets are shuffled together at the start of every epoch.  Padding per batch is bounded by the bucket width,
    which is what keeps the padded [B, Tmax, F] device batches of `collate_fn_with_eos_bos` dense.

    Reference quirks kept on purpose (they change which batches come out):
      * `short_first` is accepted and ignored (bucket.py:28 overwrites it with False);
      * in frame-budget mode an utterance longer than the budget that comes first in its bucket emits an EMPTY batch
        before it (bucket.py:139-142), and `drop_last` drops the last partial batch of every bucket;
      * the per-bucket lists are shuffled in place, so `shuffle_batch_in_bucket()` (called between epochs) reshuffles the
        previous epoch's order rather than the dataset order.
    Bucket lookup is one `np.searchsorted` over all lengths instead of a numpy round trip per utterance."""
    INT32_MAX = int(np.iinfo(np.int32).max)

    def __init__(self, dataset, bucket_boundaries, bucket_batch_size=[], rm_the_long_sents=True,
                 audo_set_batch_size=True, max_frames_one_batch=20000, drop_last=False, short_first=False):
        assert isinstance(bucket_boundaries, list) and isinstance(bucket_batch_size, list)
        self.index_length_pair = list(dataset.index_length_pair())
        self.bucket_boundaries = bucket_boundaries
        self.bucket_batch_size = bucket_batch_size
        self.rm_the_long_sents = rm_the_long_sents
        self.audo_set_batch_size = audo_set_batch_size
        self.max_frames_one_batch = max_frames_one_batch
        self.drop_last = drop_last
        self.short_first = False
        if audo_set_batch_size:
            assert max_frames_one_batch > 0
        self.max_length = bucket_boundaries[-1] if rm_the_long_sents else self.INT32_MAX
        self.num_of_buckets = len(bucket_boundaries) + (0 if rm_the_long_sents else 1)
        self.buckets = {}
        for b in range(self.num_of_buckets):
            lo = 0 if b == 0 else bucket_boundaries[b - 1]
            hi = self.INT32_MAX if b == len(bucket_boundaries) else bucket_boundaries[b]
            size = 0 if audo_set_batch_size else bucket_batch_size[min(b, len(bucket_batch_size) - 1)]
            self.buckets[str(b)] = {'index_length_pair': [], 'batch_size': size, 'boundary': [lo, hi]}
        self.batch_list = []
        self.put_data_pair_into_buckets()
        self.split_the_bucket_into_batch()

    def element_to_bucket_id(self, seq_length):
        if seq_length <= 0 or seq_length > self.INT32_MAX:
            raise ValueError('no bucket holds a sequence of length %r' % (seq_length,))
        return int(np.searchsorted(np.asarray(self.bucket_boundaries), seq_length, side='left'))

    def put_data_pair_into_buckets(self):
        pairs = self.index_length_pair
        if not pairs:
            return
        lengths = np.asarray([p[1] for p in pairs])
        keep = lengths <= self.max_length if self.rm_the_long_sents else np.ones(len(pairs), bool)
        if np.any(lengths[keep] <= 0):
            raise ValueError('no bucket holds a sequence of length <= 0')
        ids = np.searchsorted(np.asarray(self.bucket_boundaries), lengths, side='left')
        for (index, length), b, k in zip(pairs, ids, keep):
            if k:
                self.buckets[str(int(b))]['index_length_pair'].append((index, length))
        self.removed = int(len(pairs) - keep.sum())

    def split_the_bucket_into_batch(self):
        self.batch_list = []
        for bucket_id, bucket in self.buckets.items():
            pairs = bucket['index_length_pair']
            if not pairs:
                continue
            random.shuffle(pairs)
            if self.audo_set_batch_size:
                self.batch_list.extend(self.generate_batches_based_length(bucket_id, pairs))
            else:
                self.batch_list.extend(self.generate_batches(bucket_id, pairs, bucket['batch_size']))

    def generate_batches(self, bucket_id, pairs, batch_size):
        n = len(pairs)
        nb = n // batch_size if self.drop_last else -(-n // batch_size)
        return [(int(bucket_id), [i for i, _ in pairs[s * batch_size:min((s + 1) * batch_size, n)]]) for s in range(nb)]

    def generate_batches_based_length(self, bucket_id, pairs):
        out, cur, frames = [], [], 0
        for index, length in pairs:
            if frames + length > self.max_frames_one_batch:
                out.append((int(bucket_id), cur))
                cur, frames = [], 0
            cur.append(index)
            frames += length
        if cur and not self.drop_last:
            out.append((int(bucket_id), cur))
        return out

    def shuffle_batch_in_bucket(self):
        if not self.short_first:
            self.split_the_bucket_into_batch()

    def padding_waste(self):
        """fraction of padded frames over all current batches (what bucketing is for): 1 - sum(len) / sum(B * Tmax)"""
        length = dict(self.index_length_pair)
        real = padded = 0
        for _, idx in self.batch_list:
            if idx:
                ls = [length[i] for i in idx]
                real += sum(ls)
                padded += len(ls) * max(ls)
        return 1.0 - real / max(padded, 1)

    def __iter__(self):
        if not self.short_first:
            random.shuffle(self.batch_list)
        for _, index_list in self.batch_list:
            yield index_list

    def __len__(self):
        return len(self.batch_list)
