"""Backoff n-gram language model for the CTC prefix beam search (CTCRecognizer mode='beam', ngram_lm=...): the `ngram_lm` /
`alpha` / `beta` that recognize/ctc.py:22-25 hands to ctcdecode.CTCBeamDecoder, character based (one LM word per acoustic unit).

NGramLM.from_arpa reads an ARPA text file (plain or .gz) into a hash table laid out for the device: include/otrans_hip.h states the
entry layout and the scoring rule, csrc/ngram.h is the device side of this file.  The table is built with numpy; lookup_host walks
the very table the kernels probe, lookup does the same on the device (otr_ngram_lookup), and ops.ctc_prefix_beam_search_lm fuses
the model into the search."""
import gzip
import io
import math

import numpy as np

from .data import EOS

MAX_ORDER = 5
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
