"""GPU (-m gpu): otr_edit_align / otr_nbest_consensus, their wrappers, the recognizers' mbr / confidence paths and
evaluate(confidence=True) against the restatement tests/nbest_consensus_ref.py.

Integers (dist, code, ref_pos, best, which slots are dead, the zeros of conf) are compared exactly.  The float outputs against the
float64 restatement: post within 1e-6 absolute (an fp32 softmax over at most 32 terms), risk within 1e-6 * (1 + the longest
hypothesis), conf within 4e-6 (ordered sums of at most 32 products, each rounding to at most 2^-24 relative)."""
import ctypes as C

import numpy as np
import pytest
import torch

from opentransformer_amd import _lib, evaluate, ops
from opentransformer_amd import synthetic as syn
from opentransformer_amd.nn import EOS
from tests import nbest_consensus_cases as cases
from tests import nbest_consensus_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POST_TOL, CONF_TOL = 1e-6, 4e-6


def risk_tol(lengths, live):
    """1e-6 * (1 + the longest live hypothesis)"""
    return 1e-6 * (1 + int(np.max(np.where(live, np.asarray(lengths).reshape(live.shape), 0), initial=0)))


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ edit_align
def run_align(r, rl, h, hl=None, eos=-1):
    out = ops.edit_align(dev(r), dev(rl, torch.int32), dev(h), None if hl is None else dev(hl, torch.int32), eos=eos)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int8 and out[2].dtype == torch.int32
    return [t.cpu().numpy() for t in out]


def check_align(r, rl, h, hl=None, eos=-1, want=None):
    """the op against the restatement, exactly; and its dist and the counts of its codes against ops.edit_distance on the same tensors"""
    got = run_align(r, rl, h, hl, eos)
    want = ref.align_batch(r, rl, h, hl, eos) if want is None else want
    for g, w, name in zip(got, want, ('dist', 'code', 'ref_pos')):
        np.testing.assert_array_equal(g, w, err_msg=name)
    d, counts, _ = ops.edit_distance(dev(r), dev(rl, torch.int32), dev(h), None if hl is None else dev(hl, torch.int32), eos=eos)
    d, counts = d.cpu().numpy(), counts.cpu().numpy()
    np.testing.assert_array_equal(got[0], d)
    code, ok = got[1], d >= 0
    R = np.broadcast_to(np.asarray(rl).reshape(-1, 1), d.shape)
    S, I, M = (code == 1).sum(-1), (code == 2).sum(-1), (code == 0).sum(-1)
    np.testing.assert_array_equal(np.stack([S, R - M - S, I], -1)[ok], counts[ok])
    assert (code[~ok] == -1).all() and (got[2][~ok] == -1).all()
    return got


@pytest.fixture(scope='module')
def grid():
    g = cases.align_grid()
    return g, ref.align_batch(*g)


def test_align_length_grid(grid):
    """every pair of lengths around the chunk edges and at the limit, 4 symbols: the three predecessors tie all the time"""
    assert ops.NBEST_MAX_LEN == cases.MAX_LEN
    (r, rl, h, hl), want = grid
    check_align(r, rl, h, hl, want=want)


def test_align_int32_tokens_and_padding_is_never_read(grid):
    (r, rl, h, hl), want = grid
    cols = np.arange(cases.MAX_LEN)
    r2, h2 = np.where(cols[None] >= rl[:, None], h[:, 0], r), np.where(cols[None] >= hl, r, h[:, 0])[:, None]     # what would match
    got = ops.edit_align(dev(r2, torch.int32), dev(rl, torch.int64), dev(h2, torch.int32), dev(hl, torch.int64))
    for g, w, name in zip(got, want, ('dist', 'code', 'ref_pos')):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)


@pytest.mark.parametrize('N', [1, 3, 32])
def test_align_nbest_layout_strided_views_eos_and_bad_lengths(N):
    rng = np.random.default_rng(N)
    B, Lr, Lh = 3, 70, 67
    r = rng.integers(0, cases.ALPHABET, size=(B, Lr))
    rl = np.array([70, 0, 33])
    h = rng.integers(0, cases.ALPHABET, size=(B, N, Lh))
    hl = rng.integers(0, Lh + 1, size=(B, N))
    check_align(r, rl, h, hl)
    check_align(r, rl, h)                                           # hyp_len None: the full width
    check_align(r, rl, h, hl, eos=2)                                # a hypothesis ends before its first 2
    check_align(r, rl, h, None, eos=2)
    # lengths outside their widths: a reference's makes all its pairs invalid, a hypothesis's that pair
    rl_bad, hl_bad = rl.copy(), hl.copy()
    rl_bad[1] = Lr + 1
    hl_bad[0, 0], hl_bad[2, N - 1] = -1, Lh + 1
    got = check_align(r, rl_bad, h, hl_bad)
    assert (got[0][1] == -1).all() and got[0][0, 0] == -1 and got[0][2, N - 1] == -1
    # strided views: every second row of a wider buffer, columns from an offset
    rbig, hbig = dev(rng.integers(0, cases.ALPHABET, size=(2 * B, Lr + 9))), dev(rng.integers(0, cases.ALPHABET, size=(B, 2 * N, Lh + 5)))
    rv, hv = rbig[::2, 4:4 + Lr], hbig[:, ::2, 5:]
    assert not rv.is_contiguous() and not hv.is_contiguous()
    got = ops.edit_align(rv, dev(rl, torch.int32), hv, dev(hl, torch.int32))
    want = ref.align_batch(rv.cpu().numpy(), rl, hv.cpu().numpy(), hl)
    for g, w, name in zip(got, want, ('dist', 'code', 'ref_pos')):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    # [B, Lh]: N = 1, the outputs keep the N axis
    got = ops.edit_align(dev(r), dev(rl, torch.int32), dev(h[:, 0]), dev(hl[:, 0], torch.int32))
    assert got[0].shape == (B, 1) and got[1].shape == (B, 1, Lh)
    np.testing.assert_array_equal(got[1].cpu().numpy(), ref.align_batch(r, rl, h[:, :1], hl[:, :1])[1])


def raw_align(lib, r, rl, h, hl, eos=-1):
    """the C entry on poisoned outputs"""
    B, N, Lh = h.shape
    dist = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    code = torch.full((B, N, Lh), -7, dtype=torch.int8, device=DEV)
    pos = torch.full((B, N, Lh), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.otr_edit_align(_p(r), r.stride(0), _p(rl), _p(h), h.stride(0), h.stride(1), _p(hl), B, N, r.shape[1], Lh, eos, _p(dist),
                                  _p(code), _p(pos), _stream()), 'otr_edit_align')
    return dist, code, pos


def raw_consensus(lib, tokens, lengths, scores, scale, eos=-1):
    """the C entry on poisoned outputs"""
    B, N, L = tokens.shape
    post = torch.full((B, N), float('nan'), device=DEV)
    risk = torch.full((B, N), float('nan'), device=DEV)
    best = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    conf = torch.full((B, N, L), float('nan'), device=DEV)
    _lib.check(lib.otr_nbest_consensus(_p(tokens), tokens.stride(0), tokens.stride(1), _p(lengths), _p(scores), scale, B, N, L, eos,
                                       _p(post), _p(risk), _p(best), _p(conf), _stream()), 'otr_nbest_consensus')
    return post, risk, best, conf


def bits(t):
    return t.cpu().numpy().tobytes()


def test_align_writes_every_element_in_both_libraries(grid):
    (r, rl, h, hl), want = grid
    hl = hl.copy()
    hl[5, 0], hl[17, 0] = -1, cases.MAX_LEN + 1                     # invalid pairs are written too
    want = ref.align_batch(r, rl, h, hl)
    args = (dev(r), dev(rl, torch.int32), dev(h), dev(hl, torch.int32))
    outs = [raw_align(_lib.load(kind), *args) for kind in ('bf16', 'fp16')]
    for out in outs:
        for g, w, name in zip(out, want, ('dist', 'code', 'ref_pos')):
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)       # no -7 left, and the restatement's values
    assert all(bits(a) == bits(b) for a, b in zip(*outs))


# ------------------------------------------------------------------ nbest_consensus
@pytest.fixture(scope='module')
def consensus_refs():
    """per case: the inputs and the restatement's outputs, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            hand = {c['name']: c for c in cases.HAND}
            if name in hand:
                inp, scale = cases.hand_arrays(hand[name]), hand[name]['scale']
            else:
                _, B, N, lens, scale, seed = next(c for c in cases.CONSENSUS if c[0] == name)
                inp = cases.consensus_inputs(B, N, lens, seed)
            cache[name] = (inp, scale, ref.consensus(*inp, scale))
        return cache[name]
    return get


def compare_consensus(got, want, lengths):
    post, risk, best, conf = (t.cpu().numpy() for t in got)
    wpost, wrisk, wbest, wconf, live = want
    B, N, L = wconf.shape
    assert post.dtype == np.float32 and risk.dtype == np.float32 and best.dtype == np.int32 and conf.dtype == np.float32
    # the precondition of comparing `best`: no near-tie between the two lowest risks in the restatement
    assert cases.clear_of_near_ties(wrisk, None, live)
    np.testing.assert_array_equal(best, wbest)
    # dead slots, exactly
    assert (post[~live] == 0).all() and np.isposinf(risk[~live]).all() and (conf[~live] == 0).all()
    assert np.isfinite(risk[live]).all() and (post[live] > 0).all()
    # conf is exactly 0 from a hypothesis's end on
    past = np.arange(L)[None, None] >= np.asarray(lengths).reshape(B, N, 1)
    assert (conf[past & live[..., None]] == 0).all()
    perr = np.abs(post - wpost).max()
    rerr = np.abs(risk[live] - wrisk[live]).max() if live.any() else 0.0
    cerr = np.abs(conf - wconf).max() if conf.size else 0.0
    print('post err %.3g risk err %.3g (bound %.3g) conf err %.3g' % (perr, rerr, risk_tol(lengths, live), cerr))
    assert perr <= POST_TOL and rerr <= risk_tol(lengths, live) and cerr <= CONF_TOL


ALL_CASES = [c[0] for c in cases.CONSENSUS] + [c['name'] for c in cases.HAND]


@pytest.mark.parametrize('name', ALL_CASES)
def test_consensus_against_the_restatement(consensus_refs, name):
    (tokens, lengths, scores), scale, want = consensus_refs(name)
    args = (dev(tokens), dev(lengths, torch.int32), dev(scores, torch.float32))
    got = ops.nbest_consensus(*args, scale=scale)
    compare_consensus(got, want, lengths)
    hand = {c['name']: c for c in cases.HAND}.get(name)
    if hand is not None:
        assert got[2].tolist() == [hand['best']]
    # every element is written (the outputs start as NaN / -7), the same bits on a second run, and in the other library
    raws = [raw_consensus(_lib.load(kind), *args, scale) for kind in ('bf16', 'fp16', 'bf16')]
    for raw in raws:
        assert all(bits(a) == bits(b) for a, b in zip(raw, got))
    assert not any(torch.isnan(t).any() for t in (raws[0][0], raws[0][1], raws[0][3])) and (raws[0][2] >= -1).all()


@pytest.mark.parametrize('name', ['n3_long', 'n32'])
def test_consensus_dtypes_views_defaults_and_eos(consensus_refs, name):
    (tokens, lengths, scores), scale, want = consensus_refs(name)
    B, N, L = tokens.shape
    got = ops.nbest_consensus(dev(tokens), dev(lengths, torch.int32), dev(scores, torch.float32), scale=scale)
    # int32 tokens, int64 lengths, float64 scores (the wrapper narrows them), and a strided view of a wider buffer
    alt = ops.nbest_consensus(dev(tokens, torch.int32), dev(lengths, torch.int64), dev(scores.astype(np.float64)), scale=scale)
    big = torch.full((B, 2 * N, L + 7), 3, dtype=torch.int64, device=DEV)
    big[:, ::2, 7:] = dev(tokens)
    view = big[:, ::2, 7:]
    assert not view.is_contiguous()
    strided = ops.nbest_consensus(view, dev(lengths, torch.int32), dev(scores, torch.float32), scale=scale)
    for other in (alt, strided):
        assert all(bits(a) == bits(b) for a, b in zip(other, got))
    # eos in place of lengths: a hypothesis is written out to its end, then the eos; dead lengths cannot be said this way, so the dead
    # slots here are those of the scores alone
    ok = (lengths >= 0) & (lengths <= L)
    sc = np.where(ok, scores, -np.inf).astype(np.float32)
    tk = np.concatenate([tokens, np.full((B, N, 1), -1)], -1)
    for b in range(B):
        for n in range(N):
            if ok[b, n]:
                tk[b, n, lengths[b, n]] = 9
    tk = tk[:, :, :L]                                               # a full-width hypothesis has no eos and ends at the width
    ends = np.where((tk == 9).any(-1), (tk == 9).argmax(-1), L)     # where each hypothesis ends now
    assert (ends[ok] == lengths[ok]).all()
    with_eos = ops.nbest_consensus(dev(tk), None, dev(sc), scale=scale, eos=9)
    want_eos = ref.consensus(tk, None, sc, scale, eos=9)
    compare_consensus(with_eos, want_eos, ends)
    # scores None: the uniform posterior over all N slots
    uni = ops.nbest_consensus(dev(tk), None, None, eos=9)
    compare_consensus(uni, ref.consensus(tk, None, None, 1.0, eos=9), ends)


def test_consensus_under_graph_capture(consensus_refs):
    (tokens, lengths, scores), scale, _ = consensus_refs('n10')
    args = (dev(tokens), dev(lengths, torch.int32), dev(scores, torch.float32))
    eager = ops.nbest_consensus(*args, scale=scale)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        captured = ops.nbest_consensus(*args, scale=scale)
    for t in captured:
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(a) == bits(b) for a, b in zip(captured, eager))


# ------------------------------------------------------------------ recognizers
SEED = 1234
IDX2UNIT = {i: str(i) for i in range(100)}
KINDS = ['att', 'att_cached', 'att_joint', 'att_rescore', 'ctc_beam']
W, NBEST, SCALE = 5, 3, 0.7


@pytest.fixture(scope='module')
def setup():
    import opentransformer_amd as ota
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    syn.fill_state_dict_(model.state_dict(), SEED)
    with torch.no_grad():                   # a decoder of random weights ends at once: without EOS its hypotheses run to max_len
        model.decoder.output_layer.bias[EOS] = -30.0
    model = model.to(DEV).eval()
    inputs, targets = syn.synthetic_batch(batch=4, frames=120, feat_dim=80, vocab=100, tgt_len=6, seed=11, lengths=[120, 96, 104, 111],
                                          tgt_lengths=[6, 4, 5, 6])
    return model, {k: v.to(DEV) for k, v in inputs.items()}, {k: v.to(DEV) for k, v in targets.items()}


def build(model, kind, **kw):
    from opentransformer_amd.recognize import CTCRecognizer, SpeechToTextRecognizer
    if kind == 'ctc_beam':
        kw.pop('nbest', None)
        return CTCRecognizer(model, idx2unit=IDX2UNIT, mode='beam', beam_width=W, **kw)
    # max_len 8 ends the step loops (EOS is suppressed) at hypotheses of 8 tokens, which every utterance here (T' >= 23 frames) can
    # spell on its CTC head even with repeats: no hypothesis of the joint search scores -inf, and equal scores are what a host sort
    # and a device sort may order differently.  rescore=True has no step loop: max_len only bounds what is rescored, T' + 1 <= 32.
    base = dict(idx2unit=IDX2UNIT, beam_width=W, nbest=NBEST, max_len=32 if kind == 'att_rescore' else 8, ctc_weight=0.3)
    base.update(kw)
    return SpeechToTextRecognizer(model, apply_cache=kind == 'att_cached', joint_ctc=kind == 'att_joint', rescore=kind == 'att_rescore',
                                  **base)


def whole_beam(model, kind, x, m):
    """the search's final beam on the host, best score first: (tokens [B, W, L], lengths [B, W], scores f32 [B, W], eos)"""
    if kind == 'ctc_beam':
        rec = build(model, kind)
        with torch.no_grad():
            memory, memory_mask = rec._encode(x, m)
            log_probs, length = model.assistor.inference(memory, memory_mask)
            tokens, out_len, scores = rec._beam_search(log_probs, length)
        return tokens.cpu().numpy(), out_len.cpu().numpy(), scores.float().cpu().numpy(), -1
    tokens, lengths, scores = build(model, kind, nbest=W).recognize_tokens(x, m)
    return tokens.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), EOS


def risk_order(risk, scores, live, b):
    """slots by ascending risk, ties to the higher score, then the lower index; dead slots last in index order"""
    n = risk.shape[1]
    return sorted(range(n), key=lambda i: (risk[b, i], -scores[b, i] if live[b, i] else 0.0, i))


def strings_of(tokens, lengths, b, i):
    return ' '.join(IDX2UNIT[int(t)] for t in tokens[b, i, :lengths[b, i]])


@pytest.mark.parametrize('kind', KINDS)
def test_recognizers_without_mbr_are_the_parents(setup, kind):
    """mbr=False (the default) gives what a recognizer built without the new keywords gives, bit for bit"""
    model, inputs, _ = setup
    x, m = inputs['inputs'], inputs['mask']
    plain, off = build(model, kind), build(model, kind, mbr=False, mbr_scale=SCALE)
    a, b = plain.recognize(x, m), off.recognize(x, m)
    if kind == 'ctc_beam':
        assert a == b
    else:
        assert a[0] == b[0] and torch.equal(a[1], b[1])
    for s, t in zip(plain.recognize_tokens(x, m), off.recognize_tokens(x, m)):
        assert bits(s) == bits(t)


@pytest.mark.parametrize('kind', KINDS)
def test_recognizers_mbr_order_and_confidences(setup, kind):
    model, inputs, _ = setup
    x, m = inputs['inputs'], inputs['mask']
    tokens, lengths, scores, eos = whole_beam(model, kind, x, m)
    B = tokens.shape[0]
    assert tokens.shape[1] == W
    post, risk, _, conf, live = ref.consensus(tokens, lengths, scores, SCALE, eos=eos)
    # the check is not empty: every utterance has a 1-best with tokens, most of them live (the joint search scores a hypothesis of more
    # tokens than the utterance has frames -inf: a dead slot), and the beam disagrees about some of the tokens
    inside = np.arange(tokens.shape[2])[None] < lengths[:, :1]
    assert (lengths[:, 0] > 0).all() and live[:, 0].sum() >= 3 and ((conf[:, 0] < 0.999) & inside & live[:, :1]).any()
    n = 1 if kind == 'ctc_beam' else NBEST
    for mbr in (False, True):
        rec = build(model, kind, mbr=mbr, mbr_scale=SCALE)
        order = [risk_order(risk, scores, live, b) if mbr else list(range(W)) for b in range(B)]
        if mbr:
            # the precondition of comparing an order: the risks that decide the first n places are apart, or exactly equal
            for b in range(B):
                r = [risk[b, i] for i in order[b][:n + 1]]
                assert all(y == x_ or y - x_ > 1e-3 for x_, y in zip(r, r[1:])), (kind, b, r)
        want_strings = [[strings_of(tokens, lengths, b, i) for i in order[b][:n]] for b in range(B)]
        out = rec.recognize(x, m)
        if kind == 'ctc_beam':
            assert out == [s[0] for s in want_strings]
        else:
            assert out[0] == want_strings
            np.testing.assert_array_equal(out[1].numpy(), np.stack([scores[b, order[b][:n]] for b in range(B)]))
        tk, ln, sc = rec.recognize_tokens(x, m)
        assert tk.is_cuda and ln.dtype == torch.int32 and sc.dtype == torch.float32 and tk.shape[:2] == (B, n)
        assert [[strings_of(tk.cpu().numpy(), ln.cpu().numpy(), b, i) for i in range(n)] for b in range(B)] == want_strings
        # recognize_with_confidence: recognize()'s texts, the 1-best's units with the restatement's confidences, its posterior
        texts, confidences, utt_post = rec.recognize_with_confidence(x, m)
        assert texts == (out if kind == 'ctc_beam' else out[0])
        for b in range(B):
            first = order[b][0]
            text = texts[b] if kind == 'ctc_beam' else texts[b][0]
            assert [u for u, _ in confidences[b]] == text.split()
            got = np.array([c for _, c in confidences[b]])
            assert len(got) == lengths[b, first]
            assert np.abs(got - conf[b, first, :len(got)]).max(initial=0.0) <= CONF_TOL
            assert abs(float(utt_post[b]) - post[b, first]) <= POST_TOL
        assert utt_post.shape == (B,) and not utt_post.is_cuda


def test_evaluate_with_confidence(setup):
    model, inputs, targets = setup
    x, m = inputs['inputs'], inputs['mask']
    rec = build(model, 'att', mbr_scale=SCALE)
    batches = [(None, inputs, targets)]
    base = evaluate.evaluate(rec, batches)
    got = evaluate.evaluate(rec, batches, confidence=True)
    assert {k: v for k, v in got.items() if k not in ('nce', 'ece')} == base and set(got) == set(base) | {'nce', 'ece'}
    # the restatement, from the host's view of the same 1-best
    _, confidences, _ = rec.recognize_with_confidence(x, m)
    tg, tl = targets['targets'].cpu().numpy(), targets['targets_length'].cpu().numpy()
    conf, correct = [], []
    for b, items in enumerate(confidences):
        _, code, _ = ref.align(tg[b, 1:tl[b]].tolist(), [int(u) for u, _ in items])
        conf += [c for _, c in items]
        correct += [int(c == ref.MATCH) for c in code]
    nce, ece = ref.calibration(conf, correct)
    assert len(conf) > 0 and 0.0 <= got['ece'] <= 1.0
    assert abs(got['ece'] - ece) < 1e-9 and (np.isnan(nce) and np.isnan(got['nce']) or abs(got['nce'] - nce) < 1e-9)
