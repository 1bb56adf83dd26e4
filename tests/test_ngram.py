"""CPU (-m "not gpu"): the backoff n-gram LM of the CTC prefix beam search.  The ARPA parser and the packed table (NGramLM,
walked in numpy by lookup_host) against hand-computed values and against the dict-based restatement tests/ngram_ref.py; the
restated fused search (tests/ctc_prefix_lm_ref.py) against brute force over all paths; the recogniser's surface; and, for every
input the GPU comparisons use, that the restatement leaves enough utterances clear of a near-tie."""
import ctypes as C
import gzip
import io
import itertools
import math
import types

import numpy as np
import pytest

from opentransformer_amd import _lib
from opentransformer_amd.ngram import NGramLM, min_capacity
from tests import ctc_prefix_lm_ref as lmref
from tests import ngram_cases as cases
from tests.ngram_ref import LN10, RefLM, make_lm

HAND_ARPA = """\
some header text

\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.7\ta\t-0.3
-0.9\tb\t-0.2
-2.0\t<unk>\t-0.1

\\2-grams:
-0.4\t<s> a\t-0.25
-0.6\ta b\t-0.15
-0.8\tb a
-0.5\ta </s>

\\3-grams:
-0.2\t<s> a b
-0.3\ta b a

\\end\\
"""
HAND_UNITS = {0: '_', 1: 'e', 2: 'a', 3: 'b', 4: 'c'}          # V = 5: <s> is id 5, </s> is unit 1, 'c' is not in the LM
S, E, A, B_, C_ = 5, 1, 2, 3, 4


def test_hand_written_arpa_parses_and_scores():
    lm = NGramLM.from_arpa(io.StringIO(HAND_ARPA), HAND_UNITS)
    assert lm.order == 3 and lm.vocab_size == 5
    assert lm.stats['ngrams'] == [4, 4, 2] and lm.stats['dropped'] == 1          # <unk> has no unit here
    assert lm.stats['entries'] == 10 and lm.capacity == 32 and lm.stats['load'] <= 0.5
    want = [
        ((S, A), B_, -0.2),                      # full hit
        ((S, A), E, -0.25 + -0.5),               # one level: backoff(<s> a) + (a </s>)
        ((S, A), A, -0.25 + -0.3 + -0.7),        # two levels, down to the unigram
        ((B_, B_), A, -0.8),                     # (b b) is not stored: nothing added, then (b a)
        ((A, B_), A, -0.3),
        ((S,), A, -0.4),                         # the <s> context
        ((S,), B_, -0.5 + -0.9),
        ((), A, -0.7),                           # no context
        ((A,), B_, -0.6),                        # a context shorter than order-1
        ((E, S, A), B_, -0.2),                   # a longer context is cut to its last two ids
    ]
    got = lm.lookup_host([c for c, _, _ in want], [t for _, t, _ in want])
    assert got.dtype == np.float32
    for (c, t, v), g in zip(want, got):
        assert abs(g - v * LN10) <= 1e-6 * abs(v * LN10) + 1e-6, (c, t, g, v * LN10)
    oov = lm.lookup_host([(A,), (C_, B_), (B_, C_), (A, B_), ()], [C_, A, A, 0, 9])
    assert (oov == np.float32(-1000.0)).all()   # OOV token, OOV in the context (either place), the blank, an id past <s>
    assert lm.context(()) == [S] and lm.context((A,)) == [S, A] and lm.context((A, B_, A)) == [B_, A]
    with_unk = NGramLM.from_arpa(io.StringIO(HAND_ARPA), HAND_UNITS, unk_unit=4, oov_score=-7.0)
    assert with_unk.stats['dropped'] == 0
    assert abs(with_unk.lookup_host([(A,)], [C_])[0] - (-0.3 + -2.0) * LN10) < 1e-5
    assert with_unk.lookup_host([(A,)], [0])[0] == np.float32(-7.0)


def test_arpa_files_gzip_and_refusals(tmp_path):
    p = tmp_path / 'lm.arpa'
    p.write_text(HAND_ARPA)
    z = tmp_path / 'lm.arpa.gz'
    with gzip.open(z, 'wt') as f:
        f.write(HAND_ARPA)
    a, b = NGramLM.from_arpa(str(p), HAND_UNITS), NGramLM.from_arpa(z, HAND_UNITS)
    assert np.array_equal(a.table, b.table) and a.max_probe == b.max_probe
    k = tmp_path / 'lm.bin'
    k.write_bytes(b'mmap lm http://kheafield.com/code format version 5\n\0' + bytes(64))
    with pytest.raises(ValueError, match='KenLM binary'):
        NGramLM.from_arpa(str(k), HAND_UNITS)
    with pytest.raises(ValueError, match='declares'):
        NGramLM.from_arpa(io.StringIO(HAND_ARPA.replace('ngram 2=4', 'ngram 2=5')), HAND_UNITS)
    with pytest.raises(ValueError, match='6-gram'):
        NGramLM.from_arpa(io.StringIO('\\data\\\nngram 6=1\n\n\\6-grams:\n-1 a a a a a a\n\\end\\\n'), HAND_UNITS)
    with pytest.raises(ValueError, match='8192'):
        NGramLM.from_arpa(io.StringIO(HAND_ARPA), {9000: 'a'})
    with pytest.raises(ValueError, match='capacity'):
        NGramLM.from_arpa(io.StringIO(HAND_ARPA), HAND_UNITS, capacity=16)       # load would be 10/16


def every_query(V, order):
    ids = list(range(V + 1))
    ctxs = [c for n in range(order) for c in itertools.product(ids, repeat=n)]
    return [c for c in ctxs for _ in ids], [t for _ in ctxs for t in ids]


@pytest.mark.parametrize('order', [1, 2, 3, 5])
@pytest.mark.parametrize('tight', [False, True])
def test_lookup_host_equals_the_restatement_for_every_query(order, tight):
    """V = 5 units + <s>: every context of every length below the order, every token, OOV ids included; on a roomy table and on
    one of the smallest legal capacity, whose probe chains are longer than one entry"""
    V = 5
    lm, ref = cases.lm_pair(order, V, order, (14, 30, 50, 60)[:order - 1], absent=(4,), unk_unit=2, tight=tight)
    n = lm.stats['entries']
    assert n == len(ref.grams) and lm.stats['dropped'] == 1 and lm.order == order
    assert lm.capacity == (min_capacity(n) if tight else 4 * min_capacity(n)) and n / lm.capacity <= 0.5
    if tight and n >= 32:                        # order 3 and 5; the smaller tables may be collision free by luck
        assert lm.max_probe > 1
    assert n >= 32 or order < 3
    stored = lm.table[lm.table[:, 1] != 0]
    assert len(stored) == n and len(np.unique(stored[:, :2], axis=0)) == n        # every key once, nothing else
    ctxs, toks = every_query(V, order)
    got = lm.lookup_host(ctxs, toks)
    kinds = set()
    for c, t, g in zip(ctxs, toks, got):
        want = ref.cond(c, t)
        assert abs(g - want) <= 1e-6 * abs(want) + 1e-6, (c, t, g, want)
        kinds.add('oov' if want == ref.oov_score else 'hit' if c + (t,) in ref.grams else 'backoff')
    assert kinds == {'oov', 'hit', 'backoff'} or order == 1


def paths_by_string(lp, blank=0):
    """{label sequence: ln of the summed probability of every frame path that collapses to it}"""
    T, V = lp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = tuple(c for j, c in enumerate(path) if c != blank and (j == 0 or c != path[j - 1]))
        acc.setdefault(s, []).append(sum(lp[t, c] for t, c in enumerate(path)))
    return {s: max(v) + math.log(sum(math.exp(x - max(v)) for x in v)) for s, v in acc.items()}


@pytest.mark.parametrize('V,T', [(3, 1), (3, 2), (3, 3), (3, 4), (4, 2), (4, 3)])
@pytest.mark.parametrize('order', [1, 2, 3])
def test_restated_search_is_exact_when_nothing_is_pruned(V, T, order):
    """W = 32 holds every string of these sizes and K = V: the fused score of every string is
    ln sum(paths) + alpha * ln P_LM + beta * len, and lm_scores is the LM part of it"""
    rng = np.random.default_rng(10 * V + T)
    lp = rng.normal(size=(T, V)) * 2.0
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    _, grams, _ = make_lm(order, V, order, (6, 10)[:order - 1], absent=(V - 1,) if V == 4 else ())
    lm = RefLM(grams, order, V)
    alpha, beta = 0.7, 0.4
    hyps = lmref.decode_one(lp, T, 32, V, lm, alpha, beta)
    every = paths_by_string(lp)
    assert {s for s, _, _ in hyps} == set(every) and len(every) <= 32
    for s, sc, ls in hyps:
        want_lm = alpha * lm.score(s) + beta * len(s)
        assert abs(ls - want_lm) <= 1e-9 * abs(want_lm) + 1e-12, s
        assert abs(sc - (every[s] + want_lm)) <= 1e-9 * abs(sc) + 1e-9, (s, sc, every[s], want_lm)
    assert [sc for _, sc, _ in hyps] == sorted((sc for _, sc, _ in hyps), reverse=True)
    plain = lmref.decode_one(lp, T, 32, V, lm, 0.0, 0.0)
    from tests import ctc_prefix_ref
    assert [(s, sc) for s, sc, _ in plain] == ctc_prefix_ref.decode_one(lp, T, 32, V)       # no addend: the plain search


def c1_model():
    import opentransformer_amd as ota
    from opentransformer_amd import synthetic as syn
    return ota.SpeechToText(syn.c1_model(ctc_weight=0.3))


def test_recognizer_accepts_an_ngram_lm_object_and_build_recognizer_loads_a_path(tmp_path):
    from opentransformer_amd.recognize import CTCRecognizer, build_recognizer
    text, grams, idx2unit = make_lm(1, 100, 3, (50, 50), unk_unit=2)
    path = tmp_path / 'units.arpa'
    path.write_text(text)
    lm = NGramLM.from_arpa(str(path), idx2unit, unk_unit=2)
    model = c1_model()
    rec = CTCRecognizer(model, idx2unit=idx2unit, mode='beam', ngram_lm=lm, alpha=0.5, beta=1.0)
    assert rec.ngram_lm is lm and (rec.alpha, rec.beta) == (0.5, 1.0)
    with pytest.raises(NotImplementedError, match='from_arpa'):
        CTCRecognizer(model, idx2unit=idx2unit, mode='beam', ngram_lm=str(path))
    assert CTCRecognizer(model, idx2unit=idx2unit, mode='greedy', ngram_lm=lm).mode == 'greedy'     # ignored, as in the reference
    args = types.SimpleNamespace(lm_weight=0.1, ngram_lm=str(path), beam_width=4, ngpu=1, mode='beam', alpha=0.3, beta=0.2)
    built = build_recognizer('ctc', model, None, args, idx2unit)
    assert isinstance(built.ngram_lm, NGramLM) and built.ngram_lm.order == 3 and built.ngram_lm.vocab_size == 100
    assert built.ngram_lm.stats['dropped'] == 2 and (built.alpha, built.beta, built.beam_width) == (0.3, 0.2, 4)
    args.ngram_lm = None
    assert build_recognizer('ctc', model, None, args, idx2unit).ngram_lm is None


def test_entries_refuse_bad_arguments_without_a_gpu():
    import torch
    from opentransformer_amd import ops
    lib = _lib.load()
    al = C.c_void_p(4096)

    def lookup(table=al, cap=1024, max_probe=3, order=3, V=100, ctx=al, n=8):
        return lib.otr_ngram_lookup(table, cap, max_probe, order, V, ctx, al, al, n, -1000.0, al, None)
    assert lookup(cap=1000) < 0 and b'power of two' in lib.otr_last_error_string()
    assert lookup(table=C.c_void_p(4096 + 16)) < 0 and lookup(table=None) < 0
    assert lookup(order=0) < 0 and lookup(order=6) < 0 and lookup(max_probe=0) < 0 and lookup(V=8193) < 0
    assert lookup(ctx=None) < 0 and b'ngram_lookup' in lib.otr_last_error_string()
    assert lookup(n=0) == 0

    def search(W=5, K=40, cap=1024, order=3, lm_scores=al, alpha=0.5):
        ws = lib.otr_ctc_beam_workspace_bytes(2, 8, 5)
        return lib.otr_ctc_beam_search_lm(al, al, al, 2, 8, 100, K, 0, W, al, ws, al, al, al, al, cap, 3, order, alpha, 1.0, -1000.0,
                                          lm_scores, None)
    assert search(W=33) < 0 and b'ctc_beam_search_lm' in lib.otr_last_error_string()
    assert search(K=101) < 0 and search(cap=48) < 0 and search(order=6) < 0 and search(lm_scores=None) < 0
    assert search(alpha=float('nan')) < 0
    lm = cases.lm_pair(2, 5, 2, (14,), absent=(4,), unk_unit=2)[0]
    with pytest.raises(_lib.OtransHipError):
        ops.ctc_prefix_beam_search_lm(torch.zeros(1, 4, 5), torch.tensor([4]), lm, 0.5, 1.0)
    with pytest.raises(_lib.OtransHipError):
        lm.lookup([()], [1], device='cpu')


@pytest.mark.parametrize('order', cases.GOLDEN_ORDERS)
@pytest.mark.parametrize('K', cases.GOLDEN_KS)
@pytest.mark.parametrize('W', cases.GOLDEN_WS)
def test_golden_inputs_leave_three_quarters_of_the_utterances_clear(W, K, order):
    for which in range(len(cases.GOLDEN_LENGTHS)):
        gaps = cases.golden_reference(W, K, order, which)[-1]
        assert cases.clear_count(gaps) >= 3, (which, gaps)


def test_size_input_leaves_three_quarters_of_the_utterances_clear():
    lm, ref = cases.size_lm()
    assert lm.order == 3 and 18000 <= lm.stats['entries'] <= 22000
    rt, rl, rs, rlm, gaps = cases.size_reference()
    assert cases.clear_count(gaps) >= 5, gaps
    assert rl[0, 0] == 0 and rs[0, 0] == 0.0 and rlm[0, 0] == 0.0
    used = {int(v) for v in rt[rt >= 0]}
    assert any((v,) not in ref.grams for v in range(1, 4233)) and len(used) > 100
