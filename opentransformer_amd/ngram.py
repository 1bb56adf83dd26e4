"""Backoff n-gram language model for the CTC prefix beam search (CTCRecognizer mode='beam', ngram_lm=...): the `ngram_lm` /
`alpha` / `beta` that recognize/ctc.py:22-25 hands to ctcdecode.CTCBeamDecoder, character based (one LM word per acoustic unit).

NGramLM.from_arpa reads an ARPA text file (plain or .gz) into a hash table laid out for the device: include/otrans_hip.h states the
entry layout and the scoring rule, csrc/ngram.h is the device side of this file.  The table is built with numpy; lookup_host walks
the very table the kernels probe, lookup does the same on the device (otr_ngram_lookup), and ops.ctc_prefix_beam_search_lm fuses
the model into the search.

NGramLM.train estimates such a model from unit-id sentences on the device (csrc/ngramtrain.hip: interpolated modified Kneser-Ney,
the estimator include/otrans_hip.h states) and NGramLM.to_arpa writes any model back as ARPA text, so the file from_arpa starts
from can be produced here."""
import gzip
import io
import math

import numpy as np

from .data import EOS

MAX_ORDER = 5
TRAIN_MAX_ORDER = 4               # the estimator's key is the one `lo` word: four 16-bit ids (NT_MAXN of csrc/ngramtrain.hip)
FALLBACK_DISCOUNTS = (0.5, 1.0, 1.5)
MAX_VOCAB = 8192                  # ids 0 .. V (V = <s>) in 16 bits: CB_MAXV of csrc/ctcbeam.hip
OOV_SCORE = -1000.0               # ctcdecode's OOV_SCORE
_KENLM_MAGIC = b'mmap lm http://kheafield.com/code'
_U = np.uint64


def _hash(lo, hi):
    """csrc/ngram.h ng_hash on uint64 arrays (numpy's uint64 arithmetic wraps, as the device's does)"""
    with np.errstate(over='ignore'):
        z = lo ^ (hi * _U(0x9e3779b97f4a7c15))
        z = (z ^ (z >> _U(30))) * _U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U(27))) * _U(0x94d049bb133111eb)
        return z ^ (z >> _U(31))


def pack_keys(ids, lens):
    """ids int [n, <= 5] n-grams left aligned, oldest id first; lens [n] in 1 .. 5 -> (lo, hi) uint64 [n]: id w[m-1-j] at bits
    [16 j, 16 j + 16) of an 80-bit value, lo = bits 0-63, hi = bits 64-79 | m << 16"""
    ids = np.asarray(ids, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    n = ids.shape[0]
    lo, hi = np.zeros(n, _U), np.zeros(n, _U)
    for j in range(min(MAX_ORDER, ids.shape[1])):      # position j of the key <- column m-1-j
        has = lens > j
        col = np.where(has, lens - 1 - j, 0)
        v = np.where(has, ids[np.arange(n), col], 0).astype(_U)
        if j < 4:
            lo |= v << _U(16 * j)
        else:
            hi |= v
    return lo, hi | (lens.astype(_U) << _U(16))


def min_capacity(n):
    """the smallest legal capacity for n entries: a power of two, load <= 0.5"""
    cap = 2
    while cap < 2 * n:
        cap *= 2
    return cap


def unpack_keys(lo, hi=None):
    """the inverse of pack_keys: (ids int64 [n, 5] left aligned, oldest id first, lens [n]); without hi the order of a key is the
    number of its non-zero 16-bit fields (the count table of the estimator, whose ids are >= 1)"""
    lo = np.asarray(lo, _U)
    f = np.stack([(lo >> _U(16 * j)) & _U(0xffff) for j in range(4)], 1).astype(np.int64)
    if hi is None:
        f = np.concatenate([f, np.zeros((len(lo), 1), np.int64)], 1)
        lens = (f != 0).sum(1)
    else:
        hi = np.asarray(hi, _U)
        f = np.concatenate([f, (hi & _U(0xffff)).astype(np.int64)[:, None]], 1)
        lens = (hi >> _U(16)).astype(np.int64)
    ids = np.zeros((len(lo), MAX_ORDER), np.int64)
    for j in range(MAX_ORDER):                             # column m-1-j <- position j of the key
        has = lens > j
        ids[np.flatnonzero(has), (lens - 1 - j)[has]] = f[has, j]
    return ids, lens


def count_bound(lengths, order):
    """sum_b sum_i min(order, i + 1) over the len_b + 2 positions of <s> w_1 .. w_n </s>: no corpus holds more distinct n-grams"""
    P = np.asarray(lengths, np.int64) + 2
    return int(np.where(P >= order, order * P - order * (order - 1) // 2, P * (P + 1) // 2).sum())


def kn_discounts(nn):
    """modified Kneser-Ney discounts (Chen & Goodman) of one order from its count-of-counts nn[0..3] = n1 .. n4: (D1, D2, D3), or
    None where the order falls back (one of n1 .. n4 is 0, or a D_k leaves [0, k])"""
    n1, n2, n3, n4 = (int(v) for v in nn)
    if min(n1, n2, n3, n4) <= 0:
        return None
    Y = n1 / (n1 + 2.0 * n2)
    d = (1.0 - 2.0 * Y * n2 / n1, 2.0 - 3.0 * Y * n3 / n2, 3.0 - 4.0 * Y * n4 / n3)
    return d if all(0.0 <= d[k] <= k + 1 for k in range(3)) else None


def _train_corpus(tokens, lengths, V, eos, device):
    """-> (tokens int64 [n, L] on the device, lengths int32 [n] on the device, lengths on the host).  Lists are checked on the host,
    padded and uploaded once; a tensor is taken as it is (its ids are checked by the count kernel)."""
    import torch
    from ._lib import OtransHipError
    if torch.is_tensor(tokens):
        if tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise ValueError('NGramLM.train: tokens must be an int64 [n, L] tensor or a list of id lists, got %s %s'
                             % (tokens.dtype, tuple(tokens.shape)))
        n, T = tokens.shape
        if lengths is None:
            len_h = np.full(n, T, np.int64)
        else:
            len_h = (lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).astype(np.int64).reshape(-1)
        if len(len_h) != n:
            raise ValueError('NGramLM.train: %d lengths for %d sentences' % (len(len_h), n))
    else:
        sents = [np.asarray(s, np.int64).reshape(-1) for s in tokens]
        n = len(sents)
        len_h = np.array([len(s) for s in sents], np.int64)
        T = int(len_h.max()) if n else 0
        flat = np.concatenate(sents) if n else np.zeros(0, np.int64)
        if len(flat) and (flat.min() < 1 or flat.max() >= V or (flat == eos).any()):
            raise ValueError('NGramLM.train: ids inside a sentence must be in [1, V = %d) and differ from the </s> unit %d' % (V, eos))
        pad = np.zeros((n, T), np.int64)
        pad[np.arange(T)[None, :] < len_h[:, None]] = flat
        tokens = torch.from_numpy(pad)
    if n == 0:
        raise ValueError('NGramLM.train: an empty corpus')
    if len_h.min() < 0 or len_h.max() > T:
        raise ValueError('NGramLM.train: lengths must be in [0, L = %d]' % T)
    if not tokens.is_cuda and not torch.cuda.is_available():
        raise OtransHipError('NGramLM.train counts on the device and no GPU is available; there is no CPU path')
    dev = tokens.device if tokens.is_cuda else torch.device(device)
    return tokens.to(dev), torch.from_numpy(len_h.astype(np.int32)).to(dev), len_h


def _train_check(err, what):
    """read the estimator's error word (one synchronisation) and raise what it says"""
    from . import ops
    from ._lib import OtransHipError
    e = int(err.item())
    if e:
        msg = 'NGramLM.train: %s: %s' % (what, '; '.join(t for b, t in ops.NGRAM_TRAIN_ERRORS.items() if e & b))
        raise OtransHipError(msg) if e & 9 else ValueError(msg)


def _train_args(order, V, eos, table_capacity):
    if not 1 <= order <= TRAIN_MAX_ORDER:
        raise ValueError('NGramLM.train: order %d, orders 1 .. %d are estimated (from_arpa reads up to %d)'
                         % (order, TRAIN_MAX_ORDER, MAX_ORDER))
    if not 2 <= V <= MAX_VOCAB:
        raise ValueError('NGramLM.train: %d units, 2 .. %d fit' % (V, MAX_VOCAB))
    if not 1 <= eos < V:
        raise ValueError('NGramLM.train: the </s> unit %d must be in [1, V = %d)' % (eos, V))
    if table_capacity is not None and (table_capacity < 2 or table_capacity & (table_capacity - 1) or table_capacity > 1 << 31):
        raise ValueError('NGramLM.train: table_capacity %d must be a power of two in [2, 2^31]' % table_capacity)


def _sorted_grams(table):
    """the filled entries of a device count table: (index into the table, int64 on the device, in (order, key) order; keys uint64 on
    the host in that order)"""
    import torch
    idx = torch.nonzero(table[:, 0]).reshape(-1)
    keys = table[idx, 0].cpu().numpy().view(_U)
    order = (np.stack([(keys >> _U(16 * j)) & _U(0xffff) for j in range(4)], 1) != 0).sum(1)
    perm = np.lexsort((keys, order))
    return idx[torch.from_numpy(perm).to(idx.device)], keys[perm]


def count_ngrams(tokens, lengths=None, *, order=3, vocab_size, eos_unit=EOS, table_capacity=None, device='cuda'):
    """The raw and continuation counts NGramLM.train estimates from (otr_ngram_count alone), for inspection and tests: every m-gram,
    m = 1 .. order, of <s> w_1 .. w_n </s> per sentence.  Returns (ids int64 [n, order] left aligned, oldest first, lens [n],
    raw [n], cont [n]: the number of distinct (m+1)-grams that end in the gram) in (order, key) order."""
    from . import ops
    order, V, eos = int(order), int(vocab_size), int(eos_unit)
    _train_args(order, V, eos, table_capacity)
    tok, ln, len_h = _train_corpus(tokens, lengths, V, eos, device)
    cap = min_capacity(count_bound(len_h, order)) if table_capacity is None else int(table_capacity)
    table, err = ops.ngram_train_count(tok, ln, order, V, eos, cap)
    _train_check(err, 'counting')
    idx, keys = _sorted_grams(table)
    cnt = table[idx, 1].cpu().numpy().view(_U)
    ids, lens = unpack_keys(keys)
    return ids[:, :order], lens, (cnt & _U(0xffffffff)).astype(np.int64), (cnt >> _U(32)).astype(np.int64)


class NGramLM:
    """A backoff n-gram over the acoustic model's units.  Ids [0, V) are the units, V is <s>.  Attributes: order, vocab_size (V),
    oov_score, capacity, max_probe (the longest probe chain of the build: the kernels bound their probe loop by it), table
    (uint64 [capacity, 4]: key lo, key hi, f32 log-prob | f32 backoff << 32, 0), stats."""

    def __init__(self, order, vocab_size, ids, lens, logp, backoff, oov_score=OOV_SCORE, capacity=None, stats=None):
        """ids int [n, order] (left aligned, oldest first), lens [n], logp / backoff natural-log f32 [n]; duplicates keep the first"""
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('NGramLM: order %d, orders 1 .. %d are built' % (order, MAX_ORDER))
        if not 1 <= vocab_size <= MAX_VOCAB:
            raise ValueError('NGramLM: %d units, at most %d fit the 16-bit ids of the table' % (vocab_size, MAX_VOCAB))
        ids = np.asarray(ids, dtype=np.int64).reshape(-1, order)
        lens = np.asarray(lens, dtype=np.int64)
        if len(lens) and (lens.min() < 1 or lens.max() > order or ids.min() < 0 or ids.max() > vocab_size):
            raise ValueError('NGramLM: n-gram lengths must be in [1, order] and ids in [0, V]')
        lo, hi = pack_keys(ids, lens)
        key = np.stack([hi, lo], 1)
        _, first = np.unique(key, axis=0, return_index=True) if len(lens) else (None, np.zeros(0, np.int64))
        first.sort()
        lo, hi = lo[first], hi[first]
        val = (np.asarray(logp, np.float32)[first].view(np.uint32).astype(_U)
               | (np.asarray(backoff, np.float32)[first].view(np.uint32).astype(_U) << _U(32)))
        n = len(first)
        cap = min_capacity(n) if capacity is None else int(capacity)
        if cap < 2 or cap & (cap - 1) or cap < 2 * n or cap > 1 << 31:
            raise ValueError('NGramLM: capacity %d must be a power of two, at least twice the %d entries' % (cap, n))
        self.order, self.vocab_size, self.oov_score, self.capacity = int(order), int(vocab_size), float(oov_score), cap
        self.table, self.max_probe = self._build(lo, hi, val, cap)
        self.stats = dict(stats or {})
        self.stats.update(entries=n, capacity=cap, load=n / cap, max_probe=self.max_probe)
        self._dev = None

    @staticmethod
    def _build(lo, hi, val, cap):
        """linear-probing insertion, one vectorised round per probe distance: in round d every pending key tries home + d; of the
        keys that meet at a free entry the first takes it.  An entry a key passed over is full for good, so a lookup that walks
        from home to the first empty entry sees every key that could be stored there; the number of rounds is the longest chain."""
        table = np.zeros((cap, 4), _U)
        mask = _U(cap - 1)
        home = _hash(lo, hi) & mask
        pending = np.arange(len(lo))
        full = np.zeros(cap, bool)
        d = 0
        while len(pending):
            pos = ((home[pending] + _U(d)) & mask).astype(np.int64)
            free = ~full[pos]
            upos, first = np.unique(pos[free], return_index=True)
            win = pending[free][first]
            table[upos, 0], table[upos, 1], table[upos, 2] = lo[win], hi[win], val[win]
            full[upos] = True
            placed = np.zeros(len(pending), bool)
            placed[np.flatnonzero(free)[first]] = True
            pending = pending[~placed]
            d += 1
        return table, max(d, 1)

    # ------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, path_or_file, idx2unit, eos_unit=EOS, unk_unit=None, oov_score=OOV_SCORE, capacity=None):
        """Read an ARPA file (a path, plain or gzip, or an open file).  Words map to unit ids through the inverse of idx2unit;
        <s> -> V = max id + 1, </s> -> eos_unit, <unk> -> unk_unit if given; an n-gram with a word that has no unit is dropped
        (stats['dropped']).  log10 values become natural logs, rounded to f32 once."""
        lines = cls._open(path_or_file)
        V = max(idx2unit) + 1
        word2id = {str(u): int(i) for i, u in idx2unit.items()}
        word2id['<s>'] = V
        if eos_unit is not None:
            word2id['</s>'] = int(eos_unit)
        if unk_unit is not None:
            word2id['<unk>'] = int(unk_unit)
        declared, seen, rows, vals, section, in_data, dropped = {}, {}, {}, {}, 0, False, 0
        for raw in lines:
            line = raw.strip()
            if not line:
                continue
            if line.startswith('\\'):
                if line == '\\data\\':
                    in_data, section = True, 0
                elif line == '\\end\\':
                    break
                elif line.endswith('-grams:'):
                    section, in_data = int(line[1:-len('-grams:')]), False
                    if not 1 <= section <= MAX_ORDER:
                        raise ValueError('NGramLM.from_arpa: a %d-gram section; orders up to %d are built' % (section, MAX_ORDER))
                    rows.setdefault(section, [])
                    vals.setdefault(section, [])
                else:
                    raise ValueError('NGramLM.from_arpa: unknown section %r' % line)
                continue
            if in_data:
                if line.startswith('ngram '):
                    k, v = line[6:].split('=')
                    declared[int(k)] = int(v)
                continue
            if not section:
                continue                                   # free text in front of \data\
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError('NGramLM.from_arpa: %r is no %d-gram line' % (line, section))
            seen[section] = seen.get(section, 0) + 1
            try:
                ids = [word2id[w] for w in f[1:section + 1]]
            except KeyError:
                dropped += 1
                continue
            rows[section].append(ids)
            vals[section].append((float(f[0]), float(f[section + 1]) if len(f) == section + 2 else 0.0))
        if not rows:
            raise ValueError('NGramLM.from_arpa: no \\n-grams: section found')
        for m in sorted(rows):
            if m in declared and declared[m] != seen.get(m, 0):
                raise ValueError('NGramLM.from_arpa: \\data\\ declares %d %d-grams, the section holds %d'
                                 % (declared[m], m, seen.get(m, 0)))
        order = max(rows)
        ids = np.zeros((sum(len(r) for r in rows.values()), order), np.int64)
        lens = np.zeros(len(ids), np.int64)
        lv = np.zeros((len(ids), 2), np.float64)
        at = 0
        for m in sorted(rows):
            k = len(rows[m])
            if k:
                ids[at:at + k, :m] = np.asarray(rows[m], np.int64)
                lens[at:at + k] = m
                lv[at:at + k] = np.asarray(vals[m], np.float64)
            at += k
        lv *= math.log(10.0)
        stats = {'order': order, 'ngrams': [len(rows.get(m, ())) for m in range(1, order + 1)], 'dropped': dropped}
        return cls(order, V, ids, lens, lv[:, 0], lv[:, 1], oov_score=oov_score, capacity=capacity, stats=stats)

    @staticmethod
    def _open(path_or_file):
        f = open(path_or_file, 'rb') if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, '__fspath__') else path_or_file
        head = f.peek(64)[:64] if hasattr(f, 'peek') else None
        if head is None:                                   # an open text file, or a binary one that cannot peek
            first = f.read(0)
            if isinstance(first, str):
                return f
            f = io.BufferedReader(f)
            head = f.peek(64)[:64]
        if head.startswith(_KENLM_MAGIC):
            raise ValueError('NGramLM.from_arpa: this is a KenLM binary file; only ARPA text (plain or .gz) is read -- keep the '
                             '.arpa the binary was built from')
        if head[:2] == b'\x1f\x8b':
            f = gzip.GzipFile(fileobj=f)
            if f.peek(64)[:len(_KENLM_MAGIC)] == _KENLM_MAGIC:
                raise ValueError('NGramLM.from_arpa: this is a gzipped KenLM binary file; only ARPA text is read')
        return io.TextIOWrapper(f, encoding='utf-8')

    # ------------------------------------------------------------------ estimation
    @classmethod
    def train(cls, tokens, lengths=None, *, order=3, vocab_size, units=None, eos_unit=EOS, discounts=None, oov_score=OOV_SCORE,
              capacity=None, table_capacity=None, device='cuda'):
        """Estimate an interpolated modified Kneser-Ney model on the device (csrc/ngramtrain.hip; include/otrans_hip.h states the
        estimator).  tokens: an int64 [n, L] tensor (on a GPU or not, rows strided freely, anything beyond `lengths`) or a list of id
        lists; every id inside a sentence lies in [1, vocab_size) and differs from eos_unit.  A sentence is read as <s> w </s> with
        <s> = vocab_size, </s> = eos_unit; order 1 .. 4.  units: the predictable ids (default: all of [1, vocab_size)); each has a
        unigram afterwards, so none scores oov_score.  discounts [order][3] overrides the computed ones.  table_capacity: the count
        table's size (a power of two; default: load <= 0.5 at the upper bound of the number of n-grams); capacity: the scoring
        table's, as in the constructor.  stats gains sentences, tokens, ngrams (per order), discounts and fallback_orders (the orders
        on (0.5, 1, 1.5)).  There is no CPU path."""
        from . import ops
        order, V, eos = int(order), int(vocab_size), int(eos_unit)
        _train_args(order, V, eos, table_capacity)
        U = np.arange(1, V) if units is None else np.unique(np.asarray(list(units), np.int64))
        if len(U) == 0 or U.min() < 1 or U.max() >= V or eos not in U:
            raise ValueError('NGramLM.train: units must be ids in [1, V = %d) and hold the </s> unit %d' % (V, eos))
        if discounts is not None:
            discounts = [[float(v) for v in row] for row in discounts]
            if len(discounts) != order or any(len(r) != 3 or not all(0.0 <= r[k] <= k + 1 for k in range(3)) for r in discounts):
                raise ValueError('NGramLM.train: discounts must be [order = %d][3] with D_k in [0, k]' % order)
        tok, ln, len_h = _train_corpus(tokens, lengths, V, eos, device)
        cap = min_capacity(count_bound(len_h, order)) if table_capacity is None else int(table_capacity)
        table, err = ops.ngram_train_count(tok, ln, order, V, eos, cap)
        _train_check(err, 'counting')
        glob = ops.ngram_train_stats(table, order, V, err)
        g = glob.cpu().numpy()
        _train_check(err, 'statistics')
        fallback = []
        if discounts is None:
            discounts = [kn_discounts(g[4 + 4 * m:8 + 4 * m]) for m in range(order)]
            fallback = [m + 1 for m in range(order) if discounts[m] is None]
            discounts = [list(d or FALLBACK_DISCOUNTS) for d in discounts]
        logp_d, bo_d = ops.ngram_train_estimate(table, order, V, len(U), discounts, glob, err)
        _train_check(err, 'probabilities')
        idx, keys = _sorted_grams(table)
        ids, lens = unpack_keys(keys)
        logp, backoff = logp_d[idx].cpu().numpy(), bo_d[idx].cpu().numpy()
        seen = ids[lens == 1, 0]
        if not np.isin(seen[seen != V], U).all():
            raise ValueError('NGramLM.train: the corpus holds ids that `units` leaves out')
        new = np.setdiff1d(U, seen)                          # units without a count: ln(gamma(empty) / |U|)
        if len(new):
            D1 = discounts[0]
            gamma = (D1[0] * float(g[1]) + D1[1] * float(g[2]) + D1[2] * float(g[3])) / float(g[0])
            with np.errstate(divide='ignore'):
                lp_new = np.float32(np.log(np.float64(gamma / len(U))))
            keys = np.concatenate([keys, new.astype(_U)])
            ids = np.concatenate([ids, np.pad(new[:, None], ((0, 0), (0, MAX_ORDER - 1)))])
            lens = np.concatenate([lens, np.ones(len(new), np.int64)])
            logp = np.concatenate([logp, np.full(len(new), lp_new, np.float32)])
            backoff = np.concatenate([backoff, np.zeros(len(new), np.float32)])
            perm = np.lexsort((keys, lens))
            ids, lens, logp, backoff = ids[perm], lens[perm], logp[perm], backoff[perm]
        stats = {'order': order, 'ngrams': [int((lens == m).sum()) for m in range(1, order + 1)], 'sentences': len(len_h),
                 'tokens': int(len_h.sum()), 'discounts': [tuple(d) for d in discounts], 'fallback_orders': fallback,
                 'count_capacity': cap, 'count_load': float(len(idx)) / cap}
        return cls(order, V, ids[:, :order], lens, logp, backoff, oov_score=oov_score, capacity=capacity, stats=stats)

    def entries(self):
        """the stored n-grams decoded from the table: (ids int64 [n, 5] left aligned, oldest first, lens, logp f32, backoff f32),
        sorted by order, then by key"""
        t = self.table[self.table[:, 1] != 0]
        t = t[np.lexsort((t[:, 0], t[:, 1]))]
        ids, lens = unpack_keys(t[:, 0], t[:, 1])
        return (ids, lens, (t[:, 2] & _U(0xffffffff)).astype(np.uint32).view(np.float32),
                (t[:, 2] >> _U(32)).astype(np.uint32).view(np.float32))

    def to_arpa(self, path_or_file, idx2unit, eos_unit=EOS):
        """Write the model as ARPA text: to a path (gzip if it ends in .gz) or an open text file.  Works for any NGramLM, one read by
        from_arpa included: the n-grams are decoded from the table.  Id V is written <s>, eos_unit </s>, every other id as
        idx2unit[id].  log10 values carry 17 digits, so from_arpa of the file gives back the same f32 bits (the same table at the same
        capacity); the unigram <s> at ARPA's -99 is written as -99."""
        V = self.vocab_size
        if max(idx2unit) + 1 != V:
            raise ValueError('NGramLM.to_arpa: idx2unit names ids up to %d, the model has V = %d' % (max(idx2unit), V))
        ids, lens, logp, backoff = self.entries()
        word = {int(i): str(u) for i, u in idx2unit.items()}
        word[V] = '<s>'
        if eos_unit is not None:
            word[int(eos_unit)] = '</s>'
        missing = sorted(set(int(v) for r, m in zip(ids, lens) for v in r[:m]) - set(word))
        if missing:
            raise ValueError('NGramLM.to_arpa: idx2unit has no unit for the ids %s' % missing[:8])
        ln10 = math.log(10.0)
        minus99 = np.float32(-99.0 * ln10)
        if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, '__fspath__'):
            name = path_or_file.decode() if isinstance(path_or_file, bytes) else str(path_or_file)
            f = gzip.open(name, 'wt', encoding='utf-8') if name.endswith('.gz') else open(name, 'w', encoding='utf-8')
            own = True
        else:
            f, own = path_or_file, False
        try:
            f.write('\n\\data\\\n')
            for m in range(1, self.order + 1):
                f.write('ngram %d=%d\n' % (m, int((lens == m).sum())))
            for m in range(1, self.order + 1):
                f.write('\n\\%d-grams:\n' % m)
                for r in np.flatnonzero(lens == m):
                    lp = '-99' if m == 1 and ids[r, 0] == V and logp[r] == minus99 else '%.17g' % (float(logp[r]) / ln10)
                    line = lp + '\t' + ' '.join(word[int(v)] for v in ids[r, :m])
                    if m < self.order or backoff[r] != 0:
                        line += '\t%.17g' % (float(backoff[r]) / ln10)
                    f.write(line + '\n')
            f.write('\n\\end\\\n')
        finally:
            if own:
                f.close()

    # ------------------------------------------------------------------ scoring
    def context(self, prefix):
        """the LM context of a prefix: <s> followed by the prefix, cut to its last order-1 ids"""
        full = [self.vocab_size] + [int(v) for v in prefix]
        return full[len(full) - min(len(full), self.order - 1):] if self.order > 1 else []

    def _queries(self, contexts, tokens):
        n1 = max(self.order - 1, 1)
        ctx = np.zeros((len(tokens), n1), np.int32)
        ln = np.zeros(len(tokens), np.int32)
        for q, c in enumerate(contexts):
            c = [int(v) for v in c][-(self.order - 1):] if self.order > 1 else []
            ctx[q, :len(c)] = c
            ln[q] = len(c)
        if len(contexts) != len(tokens):
            raise ValueError('NGramLM: %d contexts for %d tokens' % (len(contexts), len(tokens)))
        return ctx, ln, np.asarray(tokens, np.int32).reshape(-1)

    def _find_host(self, lo, hi):
        """the probe loop of csrc/ngram.h ng_find on arrays of keys -> (found bool, logp f32, backoff f32)"""
        n = len(lo)
        mask = _U(self.capacity - 1)
        pos = (_hash(lo, hi) & mask).astype(np.int64)
        found = np.zeros(n, bool)
        val = np.zeros(n, _U)
        open_ = np.ones(n, bool)
        for _ in range(self.max_probe):
            if not open_.any():
                break
            e = self.table[pos]
            hit = open_ & (e[:, 0] == lo) & (e[:, 1] == hi)
            found |= hit
            val[hit] = e[hit, 2]
            open_ &= ~hit & (e[:, 1] != 0)
            pos = np.where(open_, (pos + 1) & int(mask), pos)
        lp = (val & _U(0xffffffff)).astype(np.uint32).view(np.float32)
        bo = (val >> _U(32)).astype(np.uint32).view(np.float32)
        return found, lp, bo

    def lookup_host(self, contexts, tokens):
        """ln P(token | context) per query, f32, by the rule of include/otrans_hip.h on the packed table in numpy: `contexts` a list
        of id sequences (V = <s>; longer than order-1 is cut to its last order-1), `tokens` their next ids"""
        ctx, ln, tok = self._queries(contexts, tokens)
        n, V = len(tok), self.vocab_size
        cols = np.arange(ctx.shape[1])[None, :]
        valid = cols < ln[:, None]
        bad = (tok < 0) | (tok > V) | (valid & ((ctx < 0) | (ctx > V))).any(1)
        safe_tok = np.where(bad, 0, tok)
        safe_ctx = np.where(valid & ~bad[:, None], ctx, 0)
        # unigram presence of the token and of every context id
        has_uni = lambda v: self._find_host(*pack_keys(v.reshape(-1, 1), np.ones(v.size, np.int64)))[0]      # noqa: E731
        oov = bad | ~has_uni(safe_tok)
        for j in range(ctx.shape[1] if self.order > 1 else 0):
            oov |= (ln > j) & ~has_uni(safe_ctx[:, j])
        out = np.full(n, self.oov_score, np.float32)
        acc = np.zeros(n, np.float32)
        done = oov.copy()
        for k in range(self.order - 1, -1, -1):           # longest context suffix first
            use = ~done & (ln >= k)
            if not use.any():
                continue
            idx = np.flatnonzero(use)
            gram = np.zeros((len(idx), k + 1), np.int64)
            for j in range(k):                             # the newest k context ids, oldest first
                gram[:, j] = safe_ctx[idx, ln[idx] - k + j]
            gram[:, k] = safe_tok[idx]
            f, lp, _ = self._find_host(*pack_keys(gram, np.full(len(idx), k + 1)))
            out[idx[f]] = acc[idx[f]] + lp[f]
            done[idx[f]] = True
            miss = idx[~f]
            if k and len(miss):
                fb, _, bo = self._find_host(*pack_keys(gram[~f, :k], np.full(len(miss), k)))
                acc[miss] += np.where(fb, bo, np.float32(0))
        return out

    def to(self, device):
        """upload the table once (cached per device); returns self"""
        import torch
        device = torch.device(device)
        if self._dev is None or self._dev.device != device:
            self._dev = torch.from_numpy(self.table.view(np.int64)).to(device)
        return self

    def device_table(self, device):
        return self.to(device)._dev

    def lookup(self, contexts, tokens, device='cuda'):
        """lookup_host on the device (otr_ngram_lookup, one thread per query): f32 tensor [n] on `device`"""
        import torch
        from . import ops
        ctx, ln, tok = self._queries(contexts, tokens)
        return ops.ngram_lookup(self, torch.from_numpy(ctx).to(device), torch.from_numpy(ln).to(device),
                                torch.from_numpy(tok).to(device))

    def score(self, tokens, lengths, alpha=1.0, beta=0.0):
        """Sentence scores on the device (otr_ngram_score_seqs): tokens int64 [..., T] on a GPU (negative = padding), lengths [...]
        -> f32 [...] = alpha * (sum_l ln P(h_l | <s> h_{<l}) + ln P(</s> | <s> h)) + beta * len(h); the empty sentence scores
        alpha * ln P(</s> | <s>).  </s> is the EOS unit, as from_arpa maps it."""
        from . import ops
        return ops.ngram_score_sequences(self, tokens, lengths, alpha, beta, eos=EOS)
