"""CPU (-m "not gpu"): phrase biasing (SpeechToTextRecognizer bias=...).  The restatement (tests/bias_ref.py) is checked against brute
force -- the addends of every string sum to its completed phrases plus what its open match holds -- PhraseBias's table and host walk
against the restatement, bit for bit; with nothing pruned every finished hypothesis of the restated search scores the n-gram fusion's
identity plus the phrase score; the recognizer and the library's entry points refuse what is outside the documented limits before
they launch."""
import ctypes as C
import itertools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib
from opentransformer_amd.bias import BIAS_MAX_LEN, PhraseBias
from tests import bias_ref as ref
from tests import ngram_attn_ref
from tests.ngram_cases import lm_pair
from tests.test_ngram_attn import att_table, collapse, rand_lp

BLANK, EOS = 0, 1
NEG = -math.inf
F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'otrans_hip.h')


def small_sets():
    """V = 4 (the units 0, 2, 3; 1 = EOS): hand-made sets with shared prefixes of different weights, a phrase that is a prefix of
    another and one that is a suffix of another, then random sets of 1-5 phrases of 1-4 ids, weights from {0.5, 1, 2}"""
    sets = [([(2, 3), (2, 3, 0), (2, 0)], [2.0, 0.5, 1.0]),                      # shared prefixes, different weights; a prefix of another
            ([(0, 2, 3), (2, 3), (3,)], [1.0, 2.0, 0.5]),                         # suffixes of another
            ([(2, 2, 2), (2, 2), (3, 2, 2, 0), (0,)], [0.5, 2.0, 1.0, 1.0])]      # repeats: a match that overlaps itself
    rng = np.random.default_rng(11)
    for _ in range(3):
        n = int(rng.integers(1, 6))
        sets.append(([tuple(int(v) for v in rng.choice([0, 2, 3], size=rng.integers(1, 5))) for _ in range(n)],
                     [float(w) for w in rng.choice([0.5, 1.0, 2.0], size=n)]))
    return sets


SMALL = small_sets()


def walk_strings(V, depth, visit, x=()):
    """every string of <= depth tokens over [0, V), a parent before its extensions"""
    visit(x)
    if len(x) < depth:
        for c in range(V):
            walk_strings(V, depth, visit, x + (c,))


@pytest.mark.parametrize('k', range(len(SMALL)))
def test_addends_sum_to_the_completed_phrases(k):
    """V = 4, every string of <= 8 tokens (EOS inside a string is a token in no phrase): the summed addends equal the banked
    completions plus psi(state); with the EOS step the banked part alone, >= 0.  Dyadic weights: exact."""
    phrases, weights = SMALL[k]
    rb = ref.RefBias(phrases, weights, 4, EOS)
    sums = {(): (0.0, 0.0)}                                                      # string -> (summed addends, banked)
    count = [0]

    def visit(x):
        if x:
            s, bank = sums[x[:-1]]
            s += float(rb.addend(x[:-1], x[-1]))
            st = rb.state(x)
            if rb.is_end(st):
                bank += float(rb.psi_minus(st))
            sums[x] = (s, bank)
        s, bank = sums[x]
        assert s == bank + float(rb.psi(rb.state(x))), x
        closed = s + float(rb.addend(x, EOS))
        assert closed == bank and closed >= 0.0, x
        count[0] += 1
    walk_strings(4, 8, visit)
    assert count[0] == sum(4 ** n for n in range(9))
    for x in ((2, 3, 0, 2), (0, 2, 2, 2, 2, 3), (3, 2, 2, 0, 2, 3, 0, 0)):        # and the helper agrees with the walk above
        got, open_ = ref.banked(rb, x)
        assert sum(float(v) for v in got) == sums[x][1] and float(open_) == float(rb.psi(rb.state(x)))
        assert float(ref.seq_score(rb, x, EOS)) == sums[x][1]


def test_the_last_16_tokens_decide_the_state():
    p16 = tuple([2, 3] * 8)
    other = (3, 3, 2)
    rb = ref.RefBias([p16, other], [1.0, 2.0], 4, EOS)
    pb = PhraseBias([p16, other], 4, weights=[1.0, 2.0])
    assert pb.max_len == BIAS_MAX_LEN == ref.MAX_LEN == 16
    for x in ((0,) + p16, (3, 0) + p16, (2, 3) + p16, (3,) + p16, p16 + (2,), p16 + (2, 3), p16[1:] + (3, 2)):
        assert len(x) in (17, 18)
        assert rb.state(x) == rb.state(x[-16:]) == pb.node_prefix(pb.walk_host(x)), x
    assert rb.state((0,) + p16) == p16 and rb.state((2, 3) + p16) == p16
    assert rb.state(p16 + (2,)) == p16[:15] and rb.state(p16[1:] + (3, 2)) == other        # 2 3 2 3 ... 2: the phrase shifted by two


@pytest.mark.parametrize('k', range(4))                       # the hand-made sets and one random one
def test_phrasebias_matches_the_restatement_on_every_string(k):
    """walk_host / addend_host on every string of <= 8 tokens over V = 4 (addend_host: every string of <= 7 and every next token),
    score_host on every string of <= 6 and on the 8-token strings that begin 2 3: the restatement's nodes and f32 bits"""
    phrases, weights = SMALL[k]
    rb = ref.RefBias(phrases, weights, 4, EOS)
    pb = PhraseBias(phrases, 4, weights=weights)
    bits = lambda v: F32(v).view(np.uint32)                    # noqa: E731

    def visit(x):
        assert pb.node_prefix(pb.walk_host(x)) == rb.state(x), x
        if len(x) < 8:
            for c in range(4):
                assert bits(pb.addend_host(x, c)) == bits(rb.addend(x, c)), (x, c)
        if len(x) <= 6 or x[:2] == (2, 3):
            assert bits(pb.score_host(x)) == bits(ref.seq_score(rb, x, EOS)), x
    walk_strings(4, 8, visit)


def big_set(seed=3, V=100, n=200):
    """200 random phrases over V = 100 incl. lengths 1 and 16, many of them extensions or tails of earlier ones, random weights"""
    rng = np.random.default_rng(seed)
    units = [v for v in range(V) if v != EOS]
    phrases = []
    for i in range(n):
        ln = (1, 16)[i] if i < 2 else int(rng.integers(1, 17))
        kind = rng.integers(0, 3) if i >= 10 else 0
        p = tuple(int(v) for v in rng.choice(units, size=ln))
        if kind == 1:                                            # shares a prefix with an earlier phrase
            q = phrases[int(rng.integers(0, len(phrases)))]
            p = (q[:int(rng.integers(1, len(q) + 1))] + p)[:ln]
        elif kind == 2:                                          # ends like an earlier phrase begins
            q = phrases[int(rng.integers(0, len(phrases)))]
            p = (p + q[:int(rng.integers(1, len(q) + 1))])[-ln:]
        phrases.append(p)
    weights = [float(F32(w)) for w in rng.uniform(0.0, 3.0, size=n)]
    return phrases, weights


def big_prefixes(rng, phrases, V, n):
    """prefixes that walk into phrases and out of them: pieces of phrases, random ids, ids outside [0, V)"""
    out = []
    for _ in range(n):
        x = []
        for _ in range(int(rng.integers(0, 5))):
            kind = rng.integers(0, 4)
            if kind == 0:
                x += [int(v) for v in rng.integers(-3, V + 3, size=rng.integers(1, 4))]
            else:
                q = phrases[int(rng.integers(0, len(phrases)))]
                a = int(rng.integers(0, len(q)))
                x += q[a:int(rng.integers(a + 1, len(q) + 1))] if kind == 1 else q[:int(rng.integers(1, len(q) + 1))]
        out.append(tuple(x))
    return out


def test_phrasebias_matches_the_restatement_at_v100():
    V = 100
    phrases, weights = big_set()
    assert {1, 16} <= {len(p) for p in phrases}
    rb = ref.RefBias(phrases, weights, V, EOS)
    pb = PhraseBias(phrases, V, weights=weights)
    rng = np.random.default_rng(5)
    deep = partial = 0
    bits = lambda v: F32(v).view(np.uint32)                    # noqa: E731
    for i, x in enumerate(big_prefixes(rng, phrases, V, 2000)):
        st = rb.state(x)
        assert pb.node_prefix(pb.walk_host(x)) == st, x
        q = phrases[int(rng.integers(0, len(phrases)))]
        nxt = [EOS, int(rng.integers(-2, V + 2)), q[0]]
        nxt += [p[len(st)] for p in phrases if len(p) > len(st) and p[:len(st)] == st][:2]      # tokens that go on
        for c in nxt:
            assert bits(pb.addend_host(x, c)) == bits(rb.addend(x, c)), (x, c)
        if i % 8 == 0:
            assert bits(pb.score_host(x)) == bits(ref.seq_score(rb, x, EOS)), x
        deep += len(st) >= 3
        partial += 0 < len(st) < len(x) and not rb.is_node(x[-len(st) - 1:])
    assert deep > 100 and partial > 300
    # the table: one entry per edge, every one within max_probe of its home
    from opentransformer_amd.bias import _hash
    used = np.flatnonzero(pb.table[:, 0])
    assert len(used) == pb.n_nodes - 1 and pb.capacity & (pb.capacity - 1) == 0 and pb.capacity >= 2 * len(used)
    home = _hash(pb.table[used, 0].astype(np.int64) - 1, pb.table[used, 1] & 0x7fffffff) & (pb.capacity - 1)
    dist = (used - home) & (pb.capacity - 1)
    assert dist.max() == pb.max_probe - 1
    for pos in used:                                             # and the probe that is bounded by it finds each of them
        node, tok = int(pb.table[pos, 0]) - 1, int(pb.table[pos, 1]) & 0x7fffffff
        child, pm, end = pb._child_host(node, tok)
        assert child == int(pb.table[pos, 2]) and pm == pb.psi_minus[child] and end == bool(pb.node_end[child])
    # per node: the definition's psi_minus / psi
    for u in rng.choice(pb.n_nodes, size=200, replace=False):
        pre = pb.node_prefix(int(u))
        assert bits(pb.psi_minus[u]) == bits(rb.psi_minus(pre)) and bits(pb.psi[u]) == bits(rb.psi(pre))
        assert bool(pb.node_end[u]) == rb.is_end(pre) and pb.node_depth[u] == len(pre)


def test_constructor_refuses_and_merges():
    ok = PhraseBias([[2, 3], (2, 3), [4]], 10, weights=[0.5, 1.5, 1.0])
    assert ok.phrases == [(2, 3), (4,)] and ok.weights == [1.5, 1.0] and ok.n_nodes == 4 and ok.max_len == 2
    assert PhraseBias([[2]], 10).weights == [2.0] and PhraseBias([[2]], 10, score=0.0).psi_minus.tolist() == [0.0, 0.0]
    for kw, what in ((dict(phrases=[]), 'empty phrase set'), (dict(phrases=[[2], []]), 'empty phrase'),
                     (dict(phrases=[list(range(2, 19))]), '16'), (dict(phrases=[[2, 10]]), 'outside'), (dict(phrases=[[-1]]), 'outside'),
                     (dict(phrases=[[2, EOS]]), 'EOS'), (dict(phrases=[[2]], weights=[-0.5]), 'negative'),
                     (dict(phrases=[[2]], weights=[float('inf')]), 'finite'), (dict(phrases=[[2]], weights=[float('nan')]), 'finite'),
                     (dict(phrases=[[2]], vocab_size=8193), '8192'), (dict(phrases=[[2], [3]], weights=[1.0]), 'weights')):
        args = dict(vocab_size=10)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            PhraseBias(**args)
    assert PhraseBias([[2]], 8192).vocab_size == 8192 and PhraseBias([list(range(2, 18))], 100).max_len == 16
    assert PhraseBias([[2, 7]], 10, eos_unit=3).eos == 3
    with pytest.raises(_lib.OtransHipError, match='CUDA/HIP'):     # like every op here: no CPU path
        ok.score(torch.zeros((2, 3), dtype=torch.int64), torch.tensor([3, 1]))


def test_from_texts():
    idx2unit = {0: '<blank>', 1: '<eos>', 2: 'a', 3: 'b', 4: 'c', 5: 'th', 6: 'e'}
    pb = PhraseBias.from_texts(['abc\n', 'th e a\t3.5\n', '\n', 'abz\n', 'th q\t1.0\n', 'cab\t0.25', 'b'], idx2unit, score=1.5)
    assert pb.phrases == [(2, 3, 4), (5, 6, 2), (4, 2, 3), (3,)] and pb.weights == [1.5, 3.5, 0.25, 1.5]
    assert pb.skipped == [('abz', ['z']), ('th q', ['q'])] and pb.vocab_size == 7
    assert PhraseBias.from_texts(['a b'], idx2unit, vocab_size=50).vocab_size == 50
    with pytest.raises(ValueError, match='no phrase'):
        PhraseBias.from_texts(['xyz'], idx2unit)
    with pytest.raises(ValueError, match='EOS'):
        PhraseBias.from_texts(['a <eos>'], idx2unit)


BRUTE_PHRASES = ([(2, 3), (2,), (3, 3, 2), (0, 2), (3, 2)], [1.0, 0.5, 2.0, 0.75, 0.3])


@pytest.mark.parametrize('with_ngram', [False, True])
@pytest.mark.parametrize('mode', ['plain', 'joint'])
def test_unpruned_search_scores_the_identity(mode, with_ngram):
    """V = 4, max_len = 3, K' = V, beam 64 >= the 4^3 strings: nothing is pruned, so every hypothesis that ended in EOS carries the
    attention, CTC and n-gram terms of tests/test_ngram_attn.py's identity plus seq_score(h), whatever path the search took.  The
    bound is that test's: 16 roundings of 2^-24 relative to the sum of the terms' magnitudes."""
    V, max_len, beam, T = 4, 3, 64, 4
    alpha, beta, lam = 0.7, 0.4, (0.3 if mode == 'joint' else 0.0)
    rb = ref.RefBias(*BRUTE_PHRASES, V, EOS)
    lm = lm_pair(2, V, 2, (6,))[1] if with_ngram else None
    table, att_fn = att_table(V, max_len, 5)
    rng = np.random.default_rng(17)
    x = rand_lp(rng, T, V)
    joint = dict(x=[x], lengths=[T], ctc_weight=lam, K=V, blank=BLANK) if mode == 'joint' else None
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        key = collapse(path)
        mass[key] = mass.get(key, 0.0) + math.exp(sum(x[t][c] for t, c in enumerate(path)))
    done = []
    ref.beam_search(att_fn, 1, beam, max_len, EOS, dict(ref=rb, K=V), ngram=dict(lm=lm, alpha=alpha, beta=beta, K=V) if lm else None,
                    joint=joint, nbest=beam, finished=done)
    seen, boosted = set(), 0
    for _, h, score in done:
        h = tuple(h)
        assert h not in seen and EOS not in h
        seen.add(h)
        terms = [(1.0 - lam) * float(table[h[:l]][c]) for l, c in enumerate(h + (EOS,))]
        if mode == 'joint':
            assert BLANK not in h and mass.get(h, 0.0) > 0.0
            terms.append(lam * math.log(mass[h]))
        if lm is not None:
            terms += [alpha * lm.score(list(h) + [EOS]), beta * len(h)]
        terms.append(float(ref.seq_score(rb, h, EOS)))
        boosted += terms[-1] > 0.0
        assert abs(score - sum(terms)) <= 16 * 2.0 ** -24 * sum(abs(v) for v in terms), (h, score, sum(terms))
    if mode == 'plain':
        assert seen == {g for n in range(max_len) for g in itertools.product((0, 2, 3), repeat=n)} and boosted >= 5
    else:
        want = {g for n in range(max_len) for g in itertools.product((2, 3), repeat=n) if mass.get(g, 0.0) > 0.0}
        assert seen == want and len(seen) >= 6 and boosted >= 3


def test_weights_zero_is_the_search_without_biasing():
    """all weights 0 and K' = V: the joint search's own restatement (without an n-gram) and the n-gram fusion's (with one), plain
    and joint: the same hypotheses, torch.equal scores"""
    from tests import ctc_prefix_score_ref as base
    V, B, beam = 6, 2, 3
    zero = ref.RefBias([(2, 3), (4,), (2, 5, 5)], [0.0, 0.0, 0.0], V, EOS)
    some = ref.RefBias([(2, 3), (4,), (2, 5, 5)], [3.0, 3.0, 3.0], V, EOS)
    _, lm = lm_pair(2, V, 2, (8,))
    ng = dict(lm=lm, alpha=0.6, beta=0.2, K=V)
    _, att_fn = att_table(V, 4, 9)
    rng = np.random.default_rng(2)
    for joint in (None, dict(x=[rand_lp(rng, 7, V) for _ in range(B)], lengths=[7, 3], ctc_weight=0.4, K=V, blank=BLANK)):
        h0, s0 = base.beam_search(att_fn, B, beam, 4, EOS, joint=joint, nbest=beam)
        h1, s1 = ref.beam_search(att_fn, B, beam, 4, EOS, dict(ref=zero, K=V), joint=joint, nbest=beam)
        assert h0 == h1 and torch.equal(s0, s1)
        h2, s2 = ngram_attn_ref.beam_search(att_fn, B, beam, 4, EOS, ng, joint=joint, nbest=beam)
        h3, s3 = ref.beam_search(att_fn, B, beam, 4, EOS, dict(ref=zero, K=V), ngram=ng, joint=joint, nbest=beam)
        assert h2 == h3 and torch.equal(s2, s3)
        h4, _ = ref.beam_search(att_fn, B, beam, 4, EOS, dict(ref=some, K=V), joint=joint, nbest=beam)
        assert h4 != h0                                           # and the phrases are consulted otherwise


def test_candidate_scorer_rules():
    """the select rules of tests/ngram_attn_ref.score_candidates: a finished row, -inf staying -inf, NaN ranking last, ties to the
    lower token; EOS behind a partial match refunds it; column 0 is BOS by position"""
    rb = ref.RefBias([(2, 3, 4), (5,)], [1.0, 0.5], 8, EOS)
    nan = float('nan')
    preds = [[EOS, 2, 3], [EOS, 2, 3], [2, 3, 6]]
    out, add, ks, ki = ref.score_candidates(rb, preds, 3, [[4, EOS, 6, 5]] * 3, [[-1.0, -2.0, NEG, nan]] * 3, EOS, flags=[0, 1, 0], beam=3)
    assert add[0] == [1.0, -2.0, -2.0, -1.5] and out[0][:3] == [0.0, -4.0, NEG] and out[0][3] != out[0][3]
    assert ks[0] == [0.0, -4.0, NEG] and ki[0] == [4, EOS, 5]                     # NaN (token 5) before -inf (token 6): the lower token
    assert add[1] == [0.0] * 4 and out[1][:3] == [-1.0, -2.0, NEG] and ks[1] == [NEG] * 3 and ki[1] == [EOS] * 3
    assert add[2] == [0.0, 0.0, 0.0, 0.5]                                         # [2 | 3 6]: column 0 is no token, the state is the root
    _, _, ks, ki = ref.score_candidates(rb, [[EOS]], 1, [[7, 6, 3]], [[-1.0, -1.0, -2.0]], EOS, beam=2)
    assert ki[0] == [6, 7] and ks[0] == [-1.0, -1.0]


# ---------------------------------------------------------------- refusals, without a GPU
def test_entry_points_refuse_bad_arguments():
    """checked on the host before any launch (no GPU needed): < 0, the entry's name and the argument in the error string, and no
    buffer touched"""
    lib = _lib.load()
    buf = np.full(256, 7.0, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 32
    p = C.c_void_p(base)

    def cands(table=p, cap=4, probe=1, nodes=2, max_len=3, V=100, preds=p, ldp=10, t=1, pos=None, idx=p, cs=p, rows=4, K=8, eos=1, out=p,
              beam=0, ks=p):
        return lib.otr_bias_score_cands(table, cap, probe, nodes, max_len, V, preds, ldp, t, pos, None, idx, cs, rows, K, eos, out, None, beam,
                                        ks, ks, None)

    def seqs(table=p, cap=4, probe=1, nodes=2, max_len=3, V=100, tok=p, ln=p, n_hyp=4, T=8, eos=1, out=p):
        return lib.otr_bias_score_seqs(table, cap, probe, nodes, max_len, V, tok, ln, n_hyp, T, eos, out, None)
    odd = C.c_void_p(base + 8)
    for fn, name in ((cands, b'bias_score_cands'), (seqs, b'bias_score_seqs')):
        for kw, word in ((dict(table=None), b'table'), (dict(table=odd), b'aligned'), (dict(cap=6), b'capacity'), (dict(cap=0), b'capacity'),
                         (dict(probe=0), b'max_probe'), (dict(probe=5), b'max_probe'), (dict(nodes=1), b'n_nodes'),
                         (dict(nodes=6), b'n_nodes'), (dict(max_len=0), b'max_len'), (dict(max_len=17), b'max_len'), (dict(V=0), b'V='),
                         (dict(V=8193), b'V='), (dict(eos=100), b'eos'), (dict(eos=-1), b'eos'), (dict(out=None), b'null')):
            assert fn(**kw) < 0, (name, kw)
            err = lib.otr_last_error_string()
            assert name in err and word in err, (kw, err)
    for kw, word in ((dict(K=33), b'K='), (dict(K=0), b'K='), (dict(beam=17, K=20), b'beam'), (dict(beam=9, K=8), b'beam'),
                     (dict(beam=-1), b'beam'), (dict(beam=4, ks=None), b'top-beam'), (dict(t=0), b't='), (dict(t=11), b't='),
                     (dict(ldp=0), b't='), (dict(rows=-1), b'rows'), (dict(preds=None), b'null'), (dict(idx=None), b'null'),
                     (dict(cs=None), b'null')):
        assert cands(**kw) < 0, kw
        err = lib.otr_last_error_string()
        assert b'bias_score_cands' in err and word in err, (kw, err)
    for kw, word in ((dict(n_hyp=-1), b'n_hyp'), (dict(T=-1), b'T='), (dict(tok=None), b'null'), (dict(ln=None), b'null')):
        assert seqs(**kw) < 0, kw
        err = lib.otr_last_error_string()
        assert b'bias_score_seqs' in err and word in err, (kw, err)
    assert cands(rows=0) == 0 and seqs(n_hyp=0) == 0                              # nothing to do: no launch
    assert (buf == 7.0).all()


def _model(ctc_weight, V=12):
    dec = SimpleNamespace(output_layer=SimpleNamespace(weight=torch.zeros(V, 4)))
    m = SimpleNamespace(decoder=dec, encoder=SimpleNamespace(), eval=lambda: m)
    if ctc_weight > 0:
        m.assistor = SimpleNamespace(blank=0)
    return m


def test_recognizer_refuses_and_accepts():
    from opentransformer_amd.recognize import SpeechToTextRecognizer, build_recognizer
    pb12, pb100 = PhraseBias([[2, 3]], 12), PhraseBias([[2, 3]], 100)
    lm12, _ = lm_pair(2, 12, 2, (20,))
    rec = SpeechToTextRecognizer(_model(0.0), beam_width=4, bias=pb12)
    assert rec.bias is pb12 and rec.bias_beam == 6 and rec.ngram_beam is None       # min(V, int(1.5 * beam))
    assert SpeechToTextRecognizer(_model(0.0, V=100), beam_width=10, bias=pb100).bias_beam == 15
    assert SpeechToTextRecognizer(_model(0.0), beam_width=4, bias=pb12, bias_beam=12).bias_beam == 12
    none = SpeechToTextRecognizer(_model(0.0), beam_width=4)
    assert none.bias is None and none.bias_beam is None
    with pytest.raises(TypeError, match='PhraseBias'):
        SpeechToTextRecognizer(_model(0.0), bias=[[2, 3]])
    with pytest.raises(TypeError, match='PhraseBias'):
        SpeechToTextRecognizer(_model(0.0), bias='phrases.txt')
    with pytest.raises(ValueError, match='units'):
        SpeechToTextRecognizer(_model(0.0, V=100), bias=pb12)
    with pytest.raises(ValueError, match='beam_width'):
        SpeechToTextRecognizer(_model(0.0, V=100), beam_width=17, bias=pb100)
    for bad in (3, 33):
        with pytest.raises(ValueError, match='bias_beam'):
            SpeechToTextRecognizer(_model(0.0, V=100), beam_width=4, bias_beam=bad, bias=pb100)
    with pytest.raises(ValueError, match='bias_beam'):
        SpeechToTextRecognizer(_model(0.0), beam_width=4, bias_beam=13, bias=pb12)             # above V
    # with an n-gram LM the two scorers share its pre-beam
    both = SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_lm=lm12, ngram_beam=8, bias=pb12)
    assert both.ngram_beam == both.bias_beam == 8
    assert SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_lm=lm12, ngram_beam=8, bias=pb12, bias_beam=8).bias_beam == 8
    with pytest.raises(ValueError, match='ngram_beam'):
        SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_lm=lm12, ngram_beam=8, bias=pb12, bias_beam=7)
    with pytest.raises(ValueError, match='ngram_beam'):
        SpeechToTextRecognizer(_model(0.0), beam_width=4, ngram_lm=lm12, bias=pb12, bias_beam=7)   # the n-gram's default is 6
    # the joint and the two-pass modes take the phrases with their own limits; bias_beam is the plain search's
    j = SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, joint_ctc=True, bias=pb12)
    assert j.ctc_beam == 6 and j.bias_beam is None
    r = SpeechToTextRecognizer(_model(0.3), ctc_weight=0.3, beam_width=4, rescore=True, bias=pb12)
    assert r.bias is pb12 and r.bias_beam is None
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.3, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1,
                           bias_phrases=pb12, bias_beam=8)
    rec = build_recognizer('speech2text', _model(0.3), None, args, None)
    assert rec.bias is pb12 and rec.bias_beam == 8
    del args.bias_phrases, args.bias_beam
    rec = build_recognizer('speech2text', _model(0.3), None, args, None)
    assert rec.bias is None and rec.bias_beam is None


def test_build_recognizer_reads_a_phrase_file(tmp_path):
    from opentransformer_amd.recognize import build_recognizer
    idx2unit = {i: u for i, u in enumerate(['<blank>', '<eos>'] + list('abcdefghij'))}
    path = tmp_path / 'phrases.txt'
    path.write_text('abc\nd e f\t4.0\nxyz\n')
    args = SimpleNamespace(lm_weight=0.1, ctc_weight=0.0, beam_width=4, nbest=1, max_len=10, penalty=0, lamda=5, ngpu=1,
                           bias_phrases=str(path), bias_score=1.25)
    rec = build_recognizer('speech2text', _model(0.0), None, args, idx2unit)
    assert isinstance(rec.bias, PhraseBias) and rec.bias.vocab_size == 12 and rec.bias_beam == 6
    assert rec.bias.phrases == [(2, 3, 4), (5, 6, 7)] and rec.bias.weights == [1.25, 4.0] and rec.bias.skipped == [('xyz', ['x', 'y', 'z'])]


def test_entries_are_in_the_header_the_binding_and_both_libraries():
    import opentransformer_amd as ota
    assert ota.PhraseBias is PhraseBias
    header = open(HEADER).read()
    assert re.search(r'#define OTR_ABI_VERSION (\d+)', header).group(1) == '608' and _lib.OTR_ABI_VERSION == 608
    still = header[header.index('still 608'):header.index('#define OTR_ABI_VERSION')]
    for name in ('otr_bias_score_cands', 'otr_bias_score_seqs'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SIGNATURES and name in still
        for kind in ('bf16', 'fp16'):
            lib = _lib.load(kind)
            assert lib.otr_version() == 608 and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES['otr_bias_score_cands']) == 22 and len(_lib.SIGNATURES['otr_bias_score_seqs']) == 13
    assert int(re.search(r'#define OTR_BIAS_MAX_LEN (\d+)', header).group(1)) == BIAS_MAX_LEN
