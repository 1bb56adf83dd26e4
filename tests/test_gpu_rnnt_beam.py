"""GPU (-m gpu): the transducer's beam search -- the kernels of csrc/rnntbeam.hip at their entries, ops.rnnt_beam and
TransducerRecognizer(mode='beam') -- against the float64 restatement of tests/rnnt_beam_ref.py on the CPU (checked against the
enumeration of every alignment by tests/test_rnnt_beam.py).

Decisions (parent, step_tok, emit, n, tokens, frames, the order of the beam) are exact: every input has its decisions at least 1e-2
wide, asserted on the CPU before the device is touched, except the deliberate ties, which the tie rule decides.  The scores of the
select entry and of ops.rnnt_beam are judged per case as err <= K * floor + tiny: err and floor the largest |score - float64| over
the slots of the case for the device and for the float32 run of the restatement, tiny = 4 * frames * eps_fp32 * (the largest
magnitude among the scores, the logits and the log-sum-exps): a score is s + (x - lse), perhaps a logaddexp, per frame -- four
roundings at the size of their operands.  K_MEASURED is the worst err / floor seen on MI355X over all cases and K
twice it, rounded up.  Every test prints what it measured before it asserts."""
import ctypes as C
import functools

import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import helpers as H
from tests import rnnt_beam_ref as br
from tests import rnnt_cases as rc
from tests import rnnt_ref as rr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
K_MEASURED = 3.36          # select V 65 W 16: 9.0e-7 against a floor of 2.7e-7; the other nine cases 0.74 .. 2.65
K = 7.0
EPS = float(torch.finfo(torch.float32).eps)
NEG = float('-inf')
ML, T_ALL, T_NOW = 6, 9, 7              # the select cases: max_len, frames, the frame the step is taken at


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- 1. select, one step, at the entry
def _histories(g, V, lengths):
    """distinct random token rows of the given lengths (None: a dead slot); at V = 2 a length names its history, so a repeated one dies"""
    seen, out = set(), []
    for n in lengths:
        y = None
        if n is not None:
            for _ in range(50):
                cand = tuple(torch.randint(1, V, (n,), generator=g).tolist())
                if cand not in seen:
                    y = cand
                    break
        if y is not None:
            seen.add(y)
        out.append(y)
    return out


def _rand_lengths(g, count):
    return [int(torch.randint(2, ML - 1, (1,), generator=g)) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def select_case(V, W, seed):
    """Six utterances at frame T_NOW.  0-2 generic (histories of length 0, 1, max_len - 1 and max_len -- which offers only its stay --
    and dead slots, in three rotations so that every W sees each), 3 ended (T_b == T_NOW: copied unchanged), 4 merges (slot 0 holds
    (1), slot 1 holds (1, k1) with k1 the best extension of slot 0, slot 2 holds (1, k2) with k2 far outside slot 0's W best), 5 the
    tie (all-zero rows, equal scores: every candidate ties and the rule alone orders them).  Rows are ld = V + 3 floats apart, so
    they start on every 4-byte offset, with NaN behind column V."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * W + V % 7)
    pats = ([0, 1, None, ML - 1, ML], [ML - 1, ML, 1, None, 0], [ML, 0, ML - 1, 2, None])
    hist = []
    for p in pats:
        hist.append(_histories(g, V, (p + _rand_lengths(g, W))[:W]))
    hist.append(_histories(g, V, ([2, None, ML, 1] + _rand_lengths(g, W))[:W]))                 # ended
    k1, k2 = 1, (2 if V > W + 3 else None)
    merge = [(1,), (1, k1), (1, k2) if k2 else None] + [None] * W
    rest = [y for y in _histories(g, V, [3] * W) if y is not None and y[:1] != (1,)]
    merge = (merge[:3] + rest + [None] * W)[:W]
    hist.append(merge)
    hist.append(([(), (1, 1)] + [None] * W)[:W])                                               # the tie
    B = len(hist)
    R, ld = B * W, V + 3
    logits = torch.full((R, ld), float('nan'))
    spread = 2.0 if W > 8 else 1.0                      # 16 slots put 17 candidates side by side: spread them, the decisions stay wide
    logits[:, :V] = torch.randn((R, V), generator=g) * 3.0 * spread
    score = -5.0 * spread * torch.rand((R,), generator=g)
    n = torch.zeros((R,), dtype=torch.int32)
    tokens = torch.zeros((R, ML), dtype=torch.int64)
    frames = torch.zeros((R, ML), dtype=torch.int32)
    for b in range(B):
        for w, y in enumerate(hist[b]):
            r = b * W + w
            if y is None:
                score[r] = NEG
                continue
            n[r] = len(y)
            tokens[r, :len(y)] = torch.tensor(y, dtype=torch.int64)
            frames[r, :len(y)] = torch.sort(torch.randperm(T_NOW, generator=g)[:len(y)])[0].to(torch.int32)
    if W >= 2:                                                                                  # the merge utterance
        r = 4 * W
        logits[r, k1] = float(logits[r, :V].max()) + 1.0
        score[r], score[r + 1] = -1.0, -1.5
        if k2 and W >= 3:
            logits[r, k2] = float(logits[r, :V].min()) - 1.0
            score[r + 2] = -0.75
    r = 5 * W                                                                                   # the tie utterance
    logits[r:r + W, :V] = 0.0
    score[r:r + min(W, 2)] = -0.25
    enc_len = torch.tensor([T_ALL, T_ALL, T_ALL, T_NOW, T_ALL, T_ALL], dtype=torch.int32)
    return dict(V=V, W=W, B=B, ld=ld, logits=logits, score=score, n=n, tokens=tokens, frames=frames, enc_len=enc_len)


def select_reference(c, dtype):
    """per utterance the restatement's step (None for the ended one)"""
    W, V = c['W'], c['V']
    out = []
    for b in range(c['B']):
        sl = slice(b * W, (b + 1) * W)
        if int(c['enc_len'][b]) <= T_NOW:
            out.append(None)
            continue
        out.append(br.beam_step_ref(c['logits'][sl, :V].to(dtype), T_NOW, c['score'][sl].to(dtype), c['n'][sl], c['tokens'][sl], c['frames'][sl], ML))
    return out


def _width(o):
    """the narrowest decision of a step: candidate W against W + 1, and the neighbours of the new beam"""
    s = [float(x) for x in o['score'] if float(x) > NEG]
    return min([o['gap']] + [a - b for a, b in zip(s, s[1:])])


SELECT_SEEDS = {(65, 3): 2, (65, 16): 7, (4233, 16): 86}       # picked on the CPU: the first seed whose decisions are all wide; 0 elsewhere


@pytest.mark.parametrize('W', [1, 3, 16])
@pytest.mark.parametrize('V', [2, 65, 4233])
def test_select_entry_takes_one_step_from_poisoned_buffers(V, W):
    from opentransformer_amd import _lib as L
    c = select_case(V, W, SELECT_SEEDS.get((V, W), 0))
    want, want32 = select_reference(c, torch.float64), select_reference(c, torch.float32)
    # before the device is touched: every decision is wide but the tie's, and the case holds what it is there for
    widths = [_width(o) for b, o in enumerate(want) if o is not None and b != 5]
    print('select V %d W %d: narrowest decision %.4f, merges %s' % (V, W, min(widths), [o['merges'] if o else None for o in want]))
    assert min(widths) >= 1e-2, widths
    assert want[3] is None and _width(want[5]) == 0.0
    assert bool((c['score'] == NEG).any()) or W == 1
    if W >= 2:
        assert want[4]['merges'] >= (2 if W >= 3 and V > W + 3 else 1)
        lp0 = c['logits'][4 * W, :V].double()
        assert int((lp0[1:] > lp0[1]).sum()) == 0                                              # k1 is among slot 0's W best
        if W >= 3 and V > W + 3:
            assert int((lp0[1:] > lp0[2]).sum()) >= W                                          # k2 is not
    R, ld, B = c['B'] * W, c['ld'], c['B']
    dev = {k: c[k].to(DEV) for k in ('logits', 'score', 'n', 'tokens', 'frames', 'enc_len')}
    score_o = torch.full((R,), float('nan'), device=DEV)
    n_o, parent, emit = (torch.full((R,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    tokens_o = torch.full((R, ML), -7, dtype=torch.int64, device=DEV)
    frames_o = torch.full((R, ML), -7, dtype=torch.int32, device=DEV)
    step_tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    lib = L.load()
    L.check(lib.otr_rnnt_beam_select(_p(dev['logits']), ld, _p(dev['enc_len']), B, W, T_ALL, T_NOW, V, 0, ML, _p(dev['score']), _p(dev['n']),
                                     _p(dev['tokens']), _p(dev['frames']), _p(score_o), _p(n_o), _p(tokens_o), _p(frames_o), _p(parent),
                                     _p(step_tok), _p(emit), _stream()), 'otr_rnnt_beam_select')
    torch.cuda.synchronize()
    score_o, n_o, parent, emit, tokens_o, frames_o, step_tok = (x.cpu() for x in (score_o, n_o, parent, emit, tokens_o, frames_o, step_tok))
    err = floor = big = 0.0
    for b in range(B):
        sl = slice(b * W, (b + 1) * W)
        o = want[b]
        if o is None:                                                                           # carried over unchanged
            assert torch.equal(score_o[sl], c['score'][sl]) and torch.equal(n_o[sl], c['n'][sl]), b
            assert parent[sl].tolist() == list(range(W)) and step_tok[sl].tolist() == [0] * W and emit[sl].tolist() == [0] * W, b
            got_t = [tokens_o[b * W + w, :int(c['n'][b * W + w])].tolist() for w in range(W)]
            got_f = [frames_o[b * W + w, :int(c['n'][b * W + w])].tolist() for w in range(W)]
            assert got_t == [c['tokens'][b * W + w, :int(c['n'][b * W + w])].tolist() for w in range(W)], b
            assert got_f == [c['frames'][b * W + w, :int(c['n'][b * W + w])].tolist() for w in range(W)], b
        else:
            assert parent[sl].tolist() == o['parent'], (b, parent[sl].tolist(), o['parent'])
            assert step_tok[sl].tolist() == o['step_tok'], (b, step_tok[sl].tolist(), o['step_tok'])
            assert emit[sl].tolist() == o['emit'] and n_o[sl].tolist() == o['n'], (b, emit[sl].tolist(), n_o[sl].tolist(), o['n'])
            for w in range(W):
                assert tokens_o[b * W + w, :o['n'][w]].tolist() == o['tokens'][w] and frames_o[b * W + w, :o['n'][w]].tolist() == o['frames'][w], (b, w)
            live = o['score'] > NEG
            assert torch.equal(score_o[sl] == NEG, ~live) and bool(torch.isfinite(score_o[sl][live]).all()), (b, score_o[sl])
            if bool(live.any()):
                err = max(err, float((score_o[sl][live].double() - o['score'][live]).abs().max()))
                floor = max(floor, float((want32[b]['score'][live].double() - o['score'][live]).abs().max()))
                rows = c['logits'][sl, :V].double()
                big = max(big, float(o['score'][live].abs().max()), float(rows.abs().max()), float(torch.logsumexp(rows, -1).abs().max()))
        for w in range(W):                                                                      # nothing is written behind a length
            r = b * W + w
            assert bool((tokens_o[r, int(n_o[r]):] == -7).all()) and bool((frames_o[r, int(n_o[r]):] == -7).all()), (b, w)
    tiny = 4 * EPS * big
    print('select V %d W %d: err %.3e floor %.3e tiny %.3e err/floor %.3f' % (V, W, err, floor, tiny, err / floor if floor else float('nan')))
    assert err <= K * floor + tiny, (err, floor, tiny)


# ---------------------------------------------------------------------------------------------- 2. gather
def test_gather_reseats_every_item_bit_for_bit():
    """rows of 4, 260 and 4096 bytes; 17 items, which takes two calls; a permutation, a fan-out (one parent feeding all W slots) and
    the identity; a parent outside [0, W) never leaves the utterance's slots"""
    from opentransformer_amd import _lib as L
    B, W = 3, 4
    R = B * W
    g = torch.Generator().manual_seed(5)
    words = [(1, 65, 1024)[k % 3] for k in range(17)]
    src = [torch.randint(-2 ** 31, 2 ** 31 - 1, (R, w), generator=g, dtype=torch.int64).to(torch.int32).to(DEV) for w in words]
    dst = [torch.full((R, w), -7, dtype=torch.int32, device=DEV) for w in words]
    parent = torch.tensor([2, 0, 3, 1, 1, 1, 1, 1, 0, 1, 2, 3], dtype=torch.int32)
    lib = L.load()
    par = parent.to(DEV)
    for i, j in ((0, 16), (16, 17)):
        sp = (C.c_void_p * (j - i))(*[x.data_ptr() for x in src[i:j]])
        dp = (C.c_void_p * (j - i))(*[x.data_ptr() for x in dst[i:j]])
        nb = (C.c_int32 * (j - i))(*[4 * w for w in words[i:j]])
        L.check(lib.otr_rnnt_beam_gather(_p(par), sp, dp, nb, j - i, B, W, _stream()), 'otr_rnnt_beam_gather')
    torch.cuda.synchronize()
    rows = (torch.arange(R) // W) * W + parent.long()
    for k in range(17):
        assert torch.equal(dst[k].cpu(), src[k].cpu()[rows]), k


# ---------------------------------------------------------------------------------------------- 3. ops.rnnt_beam on the enumeration
ENUM_SEED = 0


@functools.lru_cache(maxsize=None)
def enum_case(seed):
    """V 3, W 16, B 2 with T_b 3 and 1: the table-driven transducer of tests/rnnt_beam_ref.py, float32 values"""
    pe0, table, weight, bias = br.table_model(seed=seed, dtype=torch.float32)
    pe1 = br.table_model(seed=seed + 100, dtype=torch.float32)[0]
    return torch.stack((pe0, pe1)), table, weight, bias


def _enum_reference(seed, dtype):
    pe, table, weight, bias = (x.to(dtype) for x in enum_case(seed))
    predict, joint = br.table_callbacks(table, weight, bias)
    return [br.rnnt_beam_ref(pe[b], Tb, predict, joint, 16, 50) for b, Tb in ((0, 3), (1, 1))], \
        [br.enumerate_ref(pe[b], Tb, predict, joint, 3) for b, Tb in ((0, 3), (1, 1))]


def test_rnnt_beam_scores_equal_the_enumeration_of_every_alignment():
    from opentransformer_amd import ops
    pe, table, weight, bias = enum_case(ENUM_SEED)
    (want, sums), (want32, _) = _enum_reference(ENUM_SEED, torch.float64), _enum_reference(ENUM_SEED, torch.float32)
    gap = min(w[1] for w in want)
    print('enumeration: narrowest decision %.4f, merges %s' % (gap, [w[2] for w in want]))
    assert gap >= 1e-2 and want[0][2] >= 1 and [len(w[0]) for w in want] == [15, 3]
    for b in range(2):
        for y, _, s in want[b][0]:
            assert abs(s - sums[b][tuple(y)]) <= 1e-12
    ids = table.shape[0]
    tab, wgt, bs = table.to(DEV), weight.to(DEV), bias.to(DEV)

    def predictor_step(tokens, h, c):
        hid = torch.zeros((tokens.shape[0], 1), device=DEV) if h is None else (h[0] * 2.0 + tokens.float()).clamp(max=ids - 1)
        return [hid], [hid.clone()], tab[hid.long().view(-1)].contiguous()

    def output(z):
        return (z[:, None, :] * wgt[None]).sum(-1) + bs
    ops.set_compute_dtype('fp32')
    try:
        tokens, lengths, scores, frames = ops.rnnt_beam(pe.to(DEV), torch.tensor([3, 1], dtype=torch.int32, device=DEV), predictor_step, output,
                                                        beam_width=16, max_len=50)
        torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype('bf16')
    tokens, lengths, scores, frames = tokens.cpu(), lengths.cpu(), scores.cpu(), frames.cpu()
    assert tuple(tokens.shape) == (2, 16, 50) and tokens.dtype == torch.int64 and lengths.dtype == torch.int32 and frames.dtype == torch.int32
    err = floor = big = 0.0
    for b in range(2):
        hyps = want[b][0]
        for w, (y, fr, s) in enumerate(hyps):
            assert tokens[b, w, :int(lengths[b, w])].tolist() == y and frames[b, w, :int(lengths[b, w])].tolist() == fr, (b, w)
            err, floor, big = max(err, abs(float(scores[b, w]) - s)), max(floor, abs(want32[b][0][w][2] - s)), max(big, abs(s))
        dead = slice(len(hyps), 16)
        assert bool((scores[b, dead] == NEG).all()) and int(lengths[b, dead].abs().sum()) == 0
        for w in range(16):
            assert int(tokens[b, w, int(lengths[b, w]):].abs().sum()) == 0 and int(frames[b, w, int(lengths[b, w]):].abs().sum()) == 0
    tiny = 4 * 3 * EPS * max(big, 8.0)                  # three frames; the logits and log-sum-exps of the table model stay below 8
    print('enumeration: err %.3e floor %.3e tiny %.3e err/floor %.3f' % (err, floor, tiny, err / floor if floor else float('nan')))
    assert err <= K * floor + tiny, (err, floor, tiny)


# ---------------------------------------------------------------------------------------------- 4. the recognizer against float64
BEAM_BATCH = dict(batch=4, frames=43, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[43, 7, 27, 19], tgt_lengths=[10, 8, 10, 5])
BEAM_SETTINGS = ((1, 50), (4, 50), (4, 3))             # (beam_width, max_len)
DEEP_BATCH = dict(batch=4, frames=27, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[27, 7, 19, 15], tgt_lengths=[10, 8, 10, 5])
DEEP_LAYERS = 8
UNITS = {i: 'u%d' % i for i in range(100)}
_REF = {}


def _beam_weights():
    """test_gpu_rnnt._greedy_weights' scales (the output weight x 16, the predictor projection x 4, + 10 on the blank's bias) at the
    seed a search on the CPU picked on the oracle's encoder output: every decision of every utterance at least 1e-2 wide under all
    three settings, merges, and a 2-best of another length than the 1-best"""
    own = rr.transducer_weights(seed=3)
    own['joint.output.weight'] *= 16.0
    own['joint.pred_proj.weight'] *= 4.0
    own['joint.output.bias'][0] += 10.0
    return own


def _deep_weights():
    """an 8-layer predictor (17 gather / commit items in fp32, 25 in the 16-bit modes: two calls each); the seed a search on the CPU
    picked: every decision at least 0.15 wide at W = 2, an order above what fp16 operands move a logit by"""
    own = rr.transducer_weights(seed=33, layers=DEEP_LAYERS)
    own['joint.output.weight'] *= 16.0
    own['joint.pred_proj.weight'] *= 4.0
    own['joint.output.bias'][0] += 6.0
    return own


def _oracle_memory(batch):
    from oracle import otrans_oracle as orc
    cfg = syn.c1_model(0.0)
    inputs, _ = syn.synthetic_batch(**batch)
    parts = H.filled_state(cfg, seed=21)
    with torch.no_grad():
        x, mask = orc.conv_frontend(parts['frontend'], inputs['inputs'], inputs['mask'])
        memory, mmask = orc.transformer_encoder(parts['encoder'], x, mask, cfg['encoder'])
    return memory.double(), mmask.sum(-1)


def _reference(key):
    """the float64 restatement on the oracle's encoder output, computed once: {(W, max_len): [(hyps, min_gap, merges)] per utterance}"""
    if key not in _REF:
        deep = key == 'deep'
        memory, n = _oracle_memory(DEEP_BATCH if deep else BEAM_BATCH)
        own = _deep_weights() if deep else _beam_weights()
        ref = rr.TransducerRef({k: v.double() for k, v in own.items()}, layers=DEEP_LAYERS if deep else 2)
        pe = ref.project_encoder(memory)
        out = {'frames': n.tolist()}
        for W, ml in (((2, 50),) if deep else BEAM_SETTINGS):
            out[(W, ml)] = [br.rnnt_beam_ref(pe[b], int(n[b]), ref.predict, ref.joint_logits, W, ml) for b in range(pe.shape[0])]
        _REF[key] = out
    return _REF[key]


def _load(model, own):
    parts = H.filled_state(syn.c1_model(0.0), seed=21)
    model.frontend.load_state_dict({k: v.detach() for k, v in parts['frontend'].items()}, strict=True)
    model.encoder.load_state_dict({k: v.detach() for k, v in parts['encoder'].items()}, strict=True)
    model.predictor.load_state_dict({k[len('predictor.'):]: v.detach().float() for k, v in own.items() if k.startswith('predictor.')}, strict=True)
    model.joint.load_state_dict({k[len('joint.'):]: v.detach().float() for k, v in own.items() if k.startswith('joint.')}, strict=True)
    return model


def _check_beam(rec, batch, want, W, tol, tag):
    inputs, _ = syn.synthetic_batch(**batch)
    x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
    tokens, lengths, scores, frames = (t.cpu() for t in rec._beam_search(x, m))
    worst = 0.0
    for b, (hyps, _, _) in enumerate(want):
        for w, (y, fr, s) in enumerate(hyps):
            assert tokens[b, w, :int(lengths[b, w])].tolist() == y and frames[b, w, :int(lengths[b, w])].tolist() == fr, \
                (tag, b, w, tokens[b, w, :int(lengths[b, w])].tolist(), y)
            worst = max(worst, abs(float(scores[b, w]) - s) / abs(s))
        assert bool((scores[b, len(hyps):] == NEG).all()) and int(lengths[b, len(hyps):].abs().sum()) == 0, (tag, b)
        for w in range(W):
            assert int(tokens[b, w, int(lengths[b, w]):].abs().sum()) == 0, (tag, b, w)
    print('%s: worst relative score error %.3e' % (tag, worst))
    assert worst <= tol, (tag, worst)
    return x, m, tokens, lengths, scores, frames


@pytest.mark.parametrize('W,max_len', BEAM_SETTINGS)
def test_beam_recognizer_equals_the_restatement(W, max_len):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ref = _reference('beam')
    want = ref[(W, max_len)]
    # before the device is touched
    print('beam W %d max_len %d: frames %s gap %.4f merges %d' % (W, max_len, ref['frames'], min(w[1] for w in want), sum(w[2] for w in want)))
    assert min(w[1] for w in want) >= 1e-2, [w[1] for w in want]
    assert 1 in ref['frames'] and max(ref['frames']) <= 12
    if W == 4:
        assert sum(w[2] for w in want) >= 1
        assert any(len(w[0]) > 1 and len(w[0][0][0]) != len(w[0][1][0]) for w in ref[(4, 50)])
    if max_len == 3:
        assert max(len(h[0]) for w in want for h in w[0]) == 3 < max(len(h[0]) for w in ref[(4, 50)] for h in w[0])      # truncation
    ops.set_compute_dtype('fp32')
    try:
        model = _load(ota.TransducerModel(rc.model_config()), _beam_weights()).to(DEV)
        rec = ota.TransducerRecognizer(model, UNITS, max_len=max_len, mode='beam', beam_width=W, nbest=W)
        _check_beam(rec, BEAM_BATCH, want, W, 1e-4, 'beam W %d max_len %d' % (W, max_len))
    finally:
        ops.set_compute_dtype('bf16')


# ---------------------------------------------------------------------------------------------- 5. fp16 and a deep predictor
@pytest.mark.parametrize('mode', ['fp32', 'fp16'])          # bf16 operands move a logit by about half of the 0.15 gap: no exact claim there
def test_beam_search_in_fp16_and_with_a_deep_predictor(mode):
    """the 16-bit path of the loop -- z16 from the step's joint, the twins of h in the gather and commit tables -- and tables longer
    than one call takes (17 items in fp32, 25 in fp16)"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ref = _reference('deep')
    want = ref[(2, 50)]
    print('deep: frames %s gap %.4f merges %d' % (ref['frames'], min(w[1] for w in want), sum(w[2] for w in want)))
    assert min(w[1] for w in want) >= 0.15 and sum(w[2] for w in want) >= 1, [(w[1], w[2]) for w in want]
    mc = rc.model_config()
    mc['predictor']['num_layers'] = DEEP_LAYERS
    ops.set_compute_dtype(mode)
    try:
        model = _load(ota.TransducerModel(mc), _deep_weights()).to(DEV)
        rec = ota.TransducerRecognizer(model, UNITS, max_len=50, mode='beam', beam_width=2)
        _check_beam(rec, DEEP_BATCH, want, 2, 1e-4 if mode == 'fp32' else 2e-2, 'deep ' + mode)
    finally:
        ops.set_compute_dtype('bf16')


# ---------------------------------------------------------------------------------------------- 6. the surface
def test_the_recognizer_surface_in_beam_mode():
    import opentransformer_amd as ota
    from opentransformer_amd import evaluate, ops
    inputs, targets = syn.synthetic_batch(**BEAM_BATCH)
    ops.set_compute_dtype('fp32')
    try:
        model = _load(ota.TransducerModel(rc.model_config()), _beam_weights()).to(DEV)
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        rec = ota.TransducerRecognizer(model, UNITS, max_len=50, mode='beam', beam_width=4, nbest=3)
        raw = rec._beam_search(x, m)
        again = rec._beam_search(x, m)
        assert all(torch.equal(a, b) for a, b in zip(raw, again))                               # the same bits on every run
        tok3, len3, sc3 = rec.recognize_tokens(x, m)
        assert tuple(tok3.shape) == (4, 3, 50) and tuple(len3.shape) == (4, 3) and tuple(sc3.shape) == (4, 3)
        assert torch.equal(tok3, raw[0][:, :3]) and torch.equal(len3, raw[1][:, :3]) and torch.equal(sc3, raw[2][:, :3])
        one = ota.TransducerRecognizer(model, UNITS, max_len=50, mode='beam', beam_width=4)
        tok1, len1, sc1 = one.recognize_tokens(x, m)
        assert tuple(tok1.shape) == (4, 1, 50) and tuple(len1.shape) == (4, 1) and tuple(sc1.shape) == (4, 1)
        best = [raw[0][b, 0, :int(raw[1][b, 0])].tolist() for b in range(4)]
        best_fr = [raw[3][b, 0, :int(raw[1][b, 0])].tolist() for b in range(4)]
        texts = rec.recognize(x, m)
        assert texts == rec.translate(best) and any(texts)
        texts_t, times = rec.recognize_with_times(x, m)
        assert texts_t == texts
        for b in range(4):
            assert ' '.join(u for u, _ in times[b]) == texts[b] and [t for _, t in times[b]] == best_fr[b][:len(times[b])]
        # confidences: the consensus of the raw beam
        post, _, _, conf = ops.nbest_consensus(raw[0], raw[1], raw[2], scale=1.0, eos=-1)
        ctok, clen, csc, cconf, cpost = rec.recognize_tokens_with_confidence(x, m)
        assert torch.equal(ctok, raw[0][:, :1]) and torch.equal(clen, raw[1][:, :1]) and torch.equal(csc, raw[2][:, :1])
        assert torch.equal(cpost, post[:, 0]) and torch.equal(cconf, conf[:, 0])
        texts_c, confs, utt = rec.recognize_with_confidence(x, m)
        assert texts_c == texts and torch.equal(utt, post[:, 0].cpu())
        for b in range(4):
            assert ' '.join(u for u, _ in confs[b]) == texts[b] and all(0.0 <= p <= 1.0 for _, p in confs[b])
        assert bool(((utt >= 0) & (utt <= 1)).all())
        # mbr: ascending risk, and the frames follow the tokens
        mbr = ota.TransducerRecognizer(model, UNITS, max_len=50, mode='beam', beam_width=4, nbest=4, mbr=True)
        mtok, mlen, msc, mfr = mbr._beam(x, m, 4)[:4]
        risk = ops.nbest_consensus(raw[0], raw[1], raw[2], scale=1.0, eos=-1)[1]
        order = torch.sort(risk, dim=-1, stable=True)[1]
        for b in range(4):
            for w in range(4):
                src = int(order[b, w])
                assert torch.equal(mtok[b, w], raw[0][b, src]) and torch.equal(mfr[b, w], raw[3][b, src]) and int(mlen[b, w]) == int(raw[1][b, src])
        rtok, rlen, rsc = mbr.recognize_tokens(x, m)
        assert torch.equal(rtok, mtok) and torch.equal(rlen, mlen) and torch.equal(rsc, msc)
        mt, mtimes = mbr.recognize_with_times(x, m)
        for b in range(4):
            src = int(order[b, 0])
            assert [t for _, t in mtimes[b]] == raw[3][b, src, :int(raw[1][b, src])].tolist()[:len(mtimes[b])]
        assert mt == mbr.recognize(x, m)
        out = evaluate.evaluate(rec, [(['a', 'b', 'c', 'd'], {k: v.to(DEV) for k, v in inputs.items()}, {k: v.to(DEV) for k, v in targets.items()})])
        torch.cuda.synchronize()
        assert isinstance(out, dict) and out
    finally:
        ops.set_compute_dtype('bf16')
