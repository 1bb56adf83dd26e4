"""Phrase biasing (hotwords, contextual biasing) for SpeechToTextRecognizer(bias=...) and CTCRecognizer(mode='beam', bias=...): a list
of unit-id phrases whose tokens the search boosts while a hypothesis spells one of them, and refunds when it leaves the phrase
unfinished.

PhraseBias builds the phrases' trie and the hash table of its edges with numpy; include/otrans_hip.h states the semantics and the
entry layout, csrc/bias.hip is the device side of this file (csrc/bias.h the probe it shares with the CTC prefix beam search,
ops.ctc_prefix_beam_search_bias).  walk_host / addend_host / score_host probe the very table the kernels
probe, in the kernels' order; ops.bias_score_candidates / ops.bias_score_sequences do the same on the device."""
import numpy as np

from .data import EOS

BIAS_MAX_LEN = 16                 # ids per phrase: the depth of the trie (BS_MAXLEN of csrc/bias.hip)
MAX_VOCAB = 8192                  # BS_MAXV of csrc/bias.hip, the pre-beam's limit
_U = np.uint64
_F = np.float32


def _hash(node, tok):
    """csrc/bias.hip bs_hash on integer arrays (numpy's uint64 arithmetic wraps, as the device's does) -> uint32"""
    with np.errstate(over='ignore'):
        z = ((np.asarray(node).astype(_U) << _U(16)) | np.asarray(tok).astype(_U)) * _U(0x9e3779b97f4a7c15)
        z = (z ^ (z >> _U(30))) * _U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U(27))) * _U(0x94d049bb133111eb)
        return ((z ^ (z >> _U(31))) & _U(0xffffffff)).astype(np.int64)


def min_capacity(n):
    """the smallest legal capacity for n edges: a power of two, load <= 0.5"""
    cap = 2
    while cap < 2 * n:
        cap *= 2
    return cap


class PhraseBias:
    """A phrase set over the acoustic model's units.  phrases: sequences of 1 .. 16 ids in [0, vocab_size), none of them eos_unit;
    weights: one per phrase (>= 0, finite, earned per token; default: `score` for all).  Duplicate phrases merge with the larger weight.
    Attributes: vocab_size, eos, phrases / weights (merged, in first-seen order), n_nodes (incl. the root, node 0), max_len (the longest
    phrase), node_tok / node_end / node_depth / node_parent / node_unit (the token of the edge into the node) / psi_minus / psi (per node,
    the quantities of include/otrans_hip.h), capacity, max_probe
    (the longest probe chain of the build: the kernels bound their probe loop by it) and table (uint32 [capacity, 4]: node + 1, token |
    end(child) << 31, child, the f32 bits of psi_minus(child))."""

    def __init__(self, phrases, vocab_size, score=2.0, weights=None, eos_unit=EOS, capacity=None):
        V, eos = int(vocab_size), int(eos_unit)
        if not 1 <= V <= MAX_VOCAB:
            raise ValueError('PhraseBias: %d units, V > %d does not fit the search\'s pre-beam' % (V, MAX_VOCAB))
        phrases = [tuple(int(v) for v in p) for p in phrases]
        if not phrases:
            raise ValueError('PhraseBias: an empty phrase set')
        if weights is None:
            weights = [score] * len(phrases)
        weights = [float(w) for w in weights]
        if len(weights) != len(phrases):
            raise ValueError('PhraseBias: %d weights for %d phrases' % (len(weights), len(phrases)))
        merged = {}
        for p, w in zip(phrases, weights):
            if not p:
                raise ValueError('PhraseBias: an empty phrase')
            if len(p) > BIAS_MAX_LEN:
                raise ValueError('PhraseBias: a phrase of %d ids, more than 16 do not fit (BIAS_MAX_LEN)' % len(p))
            if min(p) < 0 or max(p) >= V:
                raise ValueError('PhraseBias: the phrase %r holds an id outside [0, V = %d)' % (p, V))
            if eos in p:
                raise ValueError('PhraseBias: the phrase %r holds the EOS unit %d' % (p, eos))
            if not (w >= 0.0 and np.isfinite(w) and np.isfinite(_F(w))):
                raise ValueError('PhraseBias: the weight %r of the phrase %r is negative or not finite' % (w, p))
            merged[p] = max(merged.get(p, 0.0), w)
        self.vocab_size, self.eos = V, eos
        self.phrases, self.weights = list(merged), [merged[p] for p in merged]
        self.max_len = max(len(p) for p in self.phrases)
        # the trie: a node per distinct prefix, in the order the prefixes first appear (a parent precedes its children)
        edges = {}                                          # (node, token) -> child
        tok, end, depth, parent, unit = [_F(0)], [False], [0], [0], [-1]
        for p, w in zip(self.phrases, self.weights):
            u = 0
            for c in p:
                v = edges.get((u, c))
                if v is None:
                    v = edges[(u, c)] = len(tok)
                    tok.append(_F(0)), end.append(False), depth.append(depth[u] + 1), parent.append(u), unit.append(c)
                tok[v] = max(tok[v], _F(w))
                u = v
            end[u] = True
        n = len(tok)
        self.n_nodes = n
        self.node_tok, self.node_end = np.array(tok, _F), np.array(end, bool)
        self.node_depth, self.node_parent, self.node_unit = np.array(depth, np.int64), np.array(parent, np.int64), np.array(unit, np.int64)
        self.psi_minus, self.psi = np.zeros(n, _F), np.zeros(n, _F)
        for u in range(1, n):                               # root to leaf, f32: psi(parent) + tok(u)
            self.psi_minus[u] = self.psi[parent[u]] + self.node_tok[u]
            self.psi[u] = _F(0) if end[u] else self.psi_minus[u]
        cap = min_capacity(n - 1) if capacity is None else int(capacity)
        if cap < 2 or cap & (cap - 1) or cap < n - 1 or cap > 1 << 31:
            raise ValueError('PhraseBias: capacity %d must be a power of two, at least the %d edges' % (cap, n - 1))
        self.capacity = cap
        items = sorted(edges.items(), key=lambda kv: kv[1])
        e_node = np.array([k[0] for k, _ in items], np.int64)
        e_tok = np.array([k[1] for k, _ in items], np.int64)
        e_child = np.array([v for _, v in items], np.int64)
        self.table, self.max_probe = self._build(e_node, e_tok, e_child, cap)
        self.stats = dict(phrases=len(self.phrases), nodes=n, capacity=cap, load=(n - 1) / cap, max_probe=self.max_probe)
        self._dev = self._rows = None

    def _build(self, node, tok, child, cap):
        """linear-probing insertion, one vectorised round per probe distance (NGramLM._build): in round d every pending edge tries
        home + d, the first of those that meet at a free entry takes it; the number of rounds is the longest chain"""
        table = np.zeros((cap, 4), np.uint32)
        home = _hash(node, tok) & (cap - 1)
        pending = np.arange(len(node))
        full = np.zeros(cap, bool)
        d = 0
        while len(pending):
            pos = (home[pending] + d) & (cap - 1)
            free = ~full[pos]
            upos, first = np.unique(pos[free], return_index=True)
            win = pending[free][first]
            table[upos, 0] = node[win] + 1
            table[upos, 1] = tok[win] | (self.node_end[child[win]].astype(np.int64) << 31)
            table[upos, 2] = child[win]
            table[upos, 3] = self.psi_minus[child[win]].view(np.uint32)
            full[upos] = True
            placed = np.zeros(len(pending), bool)
            placed[np.flatnonzero(free)[first]] = True
            pending = pending[~placed]
            d += 1
        return table, max(d, 1)

    # ------------------------------------------------------------------ text
    @classmethod
    def from_texts(cls, lines, idx2unit, score=2.0, eos_unit=EOS, vocab_size=None, capacity=None):
        """One phrase per line (an iterable of strings, or an open text file), optionally a tab and its per-token weight behind it.
        The units of a phrase are separated by blanks if the line has any, else every character is a unit; they map to ids through the
        inverse of idx2unit.  A phrase with a unit outside the vocabulary is left out and listed in .skipped (as (phrase text, the
        unknown units)); empty lines are passed over.  vocab_size defaults to max(idx2unit) + 1."""
        unit2id = {str(u): int(i) for i, u in idx2unit.items()}
        V = max(idx2unit) + 1 if vocab_size is None else int(vocab_size)
        phrases, weights, skipped = [], [], []
        for raw in lines:
            line = raw.rstrip('\r\n')
            text, _, w = line.partition('\t')
            text = text.strip()
            if not text:
                continue
            units = text.split() if len(text.split()) > 1 else list(text)
            unknown = [u for u in units if u not in unit2id]
            if unknown:
                skipped.append((text, unknown))
                continue
            phrases.append([unit2id[u] for u in units])
            weights.append(float(w) if w.strip() else float(score))
        if not phrases:
            raise ValueError('PhraseBias.from_texts: no phrase is left (%d skipped for units outside the vocabulary)' % len(skipped))
        self = cls(phrases, V, weights=weights, eos_unit=eos_unit, capacity=capacity)
        self.skipped = skipped
        return self

    def node_prefix(self, u):
        """the phrase prefix that node u stands for, as a tuple of ids (the root: the empty tuple)"""
        out = []
        while u:
            out.append(int(self.node_unit[u]))
            u = int(self.node_parent[u])
        return tuple(reversed(out))

    # ------------------------------------------------------------------ the device's probing, on the host
    def _child_host(self, node, tok):
        """csrc/bias.hip bs_child on the packed table: (child, psi_minus(child), end(child)) or None"""
        if self._rows is None:                              # the table's words as Python ints, its f32 column as numpy scalars
            self._rows = (self.table.tolist(), self.table[:, 3].copy().view(_F))
        rows, pm = self._rows
        m64, mask = (1 << 64) - 1, self.capacity - 1
        z = (((node << 16) | tok) * 0x9e3779b97f4a7c15) & m64           # bs_hash, in Python's integers
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m64
        pos = ((z ^ (z >> 31)) & 0xffffffff) & mask
        for _ in range(self.max_probe):
            e = rows[pos]
            if e[0] == node + 1 and e[1] & 0x7fffffff == tok:
                return e[2], pm[pos], bool(e[1] >> 31)
            if e[0] == 0:
                return None
            pos = (pos + 1) & mask
        return None

    def _chain_host(self, prefix):
        """the suffix chain of state(prefix) as the candidate kernel's lanes find it: {j: (node, psi_minus(node), psi(node))} for every
        j <= 16 whose last j tokens are a node (j = 0: the root), read from the edges that reach the nodes"""
        x = [int(v) for v in prefix]
        chain = {0: (0, _F(0), _F(0))}
        for j in range(1, min(len(x), self.max_len) + 1):
            node, pm, psi, ok = 0, _F(0), _F(0), True
            for c in x[len(x) - j:]:
                hit = self._child_host(node, c) if 0 <= c < self.vocab_size else None
                if hit is None:
                    ok = False
                    break
                node, pm, psi = hit[0], hit[1], (_F(0) if hit[2] else hit[1])
            if ok:
                chain[j] = (node, pm, psi)
        return chain

    def walk_host(self, prefix):
        """state(prefix): the node of the longest suffix of the token string `prefix` that is a phrase prefix (0 = the root)"""
        chain = self._chain_host(prefix)
        return chain[max(chain)][0]

    def addend_host(self, prefix, c):
        """a(g, c) = psi_minus(state(g c)) - psi(state(g)) for the hypothesis whose tokens (behind BOS) are `prefix`, f32, by the
        candidate kernel's steps: the chain of g, then child(n_j, c) from the deepest j down"""
        chain = self._chain_host(prefix)
        psi_g = chain[max(chain)][2]
        pm, c = _F(0), int(c)
        if 0 <= c < self.vocab_size:
            for j in sorted(chain, reverse=True):
                hit = self._child_host(chain[j][0], c) if j < self.max_len else None
                if hit is not None:
                    pm = hit[1]
                    break
        return _F(pm - psi_g)

    def score_host(self, tokens):
        """the summed addends of tokens + [EOS], f32, in the sequence kernel's order: lane i adds the positions i, i + 64, .. in turn,
        the lane sums meet in the butterfly v_i += v_(i ^ o), o = 32 .. 1"""
        h = [int(v) for v in tokens]
        acc = np.zeros(64, _F)
        prev = _F(0)                                        # psi of the state in front of the position
        for l in range(len(h) + 1):
            pm = ps = _F(0)                                  # behind EOS: the root
            if l < len(h):
                chain = self._chain_host(h[:l + 1])
                _, pm, ps = chain[max(chain)]
            acc[l % 64] = acc[l % 64] + _F(pm - prev)
            prev = ps
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ o]
        return acc[0]

    # ------------------------------------------------------------------ device
    def to(self, device):
        """upload the table once (cached per device); returns self"""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._dev is None or self._dev.device != device:
            self._dev = torch.from_numpy(self.table.view(np.int32)).to(device)
        return self

    def device_table(self, device):
        return self.to(device)._dev

    def score(self, tokens, lengths):
        """score_host on the device (otr_bias_score_seqs): tokens int64 [..., T] on a GPU, lengths [...] -> f32 [...]"""
        from . import ops
        return ops.bias_score_sequences(self, tokens, lengths, eos=self.eos)
