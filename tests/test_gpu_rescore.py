"""GPU (-m gpu): attention rescoring of the CTC n-best (SpeechToTextRecognizer rescore=True, ops.attention_rescore, csrc/rescore.hip,
otr_dec_cross_fwd_shared) against the plain-Python restatement (tests/rescore_ref.py) on the oracle's decoder and LM."""
import math

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from oracle import otrans_oracle as orc
from tests import rescore_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EOS = 1


def _random_beam(rng, B, W, T, V, max_len):
    """a search result with ragged lengths: empty, exactly max_len - 1 tokens (n_rows = max_len), too long, dead slots, and in
    utterance 0 the same hypothesis with the same score in two slots (an exact tie of the totals)"""
    tokens = -np.ones((B, W, T), np.int64)
    out_len = np.zeros((B, W), np.int32)
    scores = -np.sort(rng.uniform(1.0, 30.0, size=(B, W)), axis=1).astype(np.float32)
    lens = [0, max_len - 1, max_len, T, 3, 5]
    for b in range(B):
        for w in range(W):
            n = lens[(b + w) % len(lens)] if w < W - 1 else 0
            out_len[b, w] = n
            tokens[b, w, :n] = rng.integers(2, V, size=n)
        scores[b, W - 1] = -np.inf                       # a dead slot: length 0, tokens -1
    out_len[0, 2] = out_len[0, 1] = 4
    tokens[0, 1] = tokens[0, 2] = -1
    tokens[0, 1, :4] = tokens[0, 2, :4] = rng.integers(2, V, size=4)
    scores[0, 2] = scores[0, 1]
    return tokens, out_len, scores


def _check_order(perm, want_total, gap=1e-4):
    """rank r holds the restatement's slot wherever the restatement's total at r is more than `gap` from both neighbours' (exact ties
    and -inf runs count as decided: they go by CTC rank)"""
    W = len(want_total)
    want = ref.order(want_total)
    t = [want_total[i] for i in want]

    def decided(a, b):
        return (a == b) or abs(a - b) > gap
    for r in range(W):
        if (r == 0 or decided(t[r - 1], t[r])) and (r == W - 1 or decided(t[r], t[r + 1])):
            assert perm[r] == want[r], (r, perm, want, t)


@pytest.mark.parametrize('V,pad', [(100, 0), (100, 4), (4233, 0), (4233, 7), (8192, 3), (8192, 0)])
@pytest.mark.parametrize('with_lm,penalty', [(False, 0.0), (True, 0.6)])
def test_kernels_match_restatement(V, pad, with_lm, penalty):
    from opentransformer_amd import ops
    rng = np.random.default_rng(V + pad)
    B, W, T, max_len, nbest = 3, 6, 14, 9, 4
    lam, mu, lamda = 0.4, 0.3, 5.0
    tokens, out_len, scores = _random_beam(rng, B, W, T, V, max_len)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    tk, ol, sc = dev(tokens), dev(out_len), dev(scores)
    packed = ops.rescore_pack(tk, ol, sc, max_len, V)
    want_in, want_out, want_rows = ref.pack(tokens, out_len, scores, max_len, V)
    assert np.array_equal(packed[0].cpu().numpy(), want_in)             # bit-exact
    assert np.array_equal(packed[1].cpu().numpy(), want_out)
    assert np.array_equal(packed[2].cpu().numpy(), want_rows)
    assert 0 in want_rows and max_len in want_rows
    ld = V + pad
    lg = (rng.normal(size=(B * W * max_len, ld)) * 3.0).astype(np.float32)
    lmg = (rng.normal(size=(B * W * max_len, ld)) * 2.0).astype(np.float32) if with_lm else None
    for a in (lg, lmg):                                                 # the tied pair sees the same rows
        if a is not None:
            a3 = a.reshape(B * W, max_len, ld)
            a3[2] = a3[1]
    lg_d = dev(lg)[:, :V] if pad else dev(lg)                           # ld > V: a view with a longer row stride
    lm_d = None if lmg is None else (dev(lmg)[:, :V] if pad else dev(lmg))
    res = ops.attention_rescore(lg_d, tk, ol, sc, max_len, V, lam, lm_logits=lm_d, lm_weight=mu, nbest=nbest, penalty=penalty, lamda=lamda,
                                packed=packed)
    again = ops.attention_rescore(lg_d, tk, ol, sc, max_len, V, lam, lm_logits=lm_d, lm_weight=mu, nbest=nbest, penalty=penalty, lamda=lamda)
    torch.cuda.synchronize()
    for k in ('att', 'lm', 'total', 'perm', 'tokens', 'len', 'scores'):
        assert (res[k] is None and again[k] is None) or torch.equal(res[k], again[k]), k      # deterministic; packing inside = packed
    att, total, perm = res['att'].cpu().numpy(), res['total'].cpu().numpy().astype(np.float64), res['perm'].cpu().numpy()
    lm_s = res['lm'].cpu().numpy() if with_lm else None
    lg3 = lg.reshape(B * W, max_len, ld)[:, :, :V].astype(np.float64)
    lm3 = lmg.reshape(B * W, max_len, ld)[:, :, :V].astype(np.float64) if with_lm else None
    beam = ref.beam_of(tokens, out_len, scores)
    want = ref.rescore(beam, lambda b, h: lg3[b * W + [s[0] for s in beam[b]].index(h)], lam, max_len,
                       lm_fn=(lambda b, h: lm3[b * W + [s[0] for s in beam[b]].index(h)]) if with_lm else None, mu=mu, penalty=penalty,
                       lamda=lamda, nbest=nbest)
    n_live = 0
    for b in range(B):
        w_ = want[b]
        for w in range(W):
            if w_['att'][w] is None:
                assert att[b, w] == -math.inf and total[b, w] == -math.inf
                continue
            n_live += 1
            # f32 sums of up to max_len rows (the bar of tests/test_gpu_joint_ctc.py for f32 sums)
            assert abs(att[b, w] - w_['att'][w]) <= 1e-4 + 1e-6 * abs(w_['att'][w]), (b, w, att[b, w], w_['att'][w])
            if with_lm:
                assert abs(lm_s[b, w] - w_['lm'][w]) <= 1e-4 + 1e-6 * abs(w_['lm'][w]), (b, w)
            assert abs(total[b, w] - w_['total'][w]) <= 1e-4 + 1e-5 * abs(w_['total'][w]), (b, w, total[b, w], w_['total'][w])
        assert sorted(perm[b].tolist()) == list(range(W))
        _check_order(perm[b].tolist(), w_['total'])
        dead = [w for w in range(W) if w_['total'][w] == -math.inf]
        assert perm[b].tolist()[W - len(dead):] == dead                   # -inf last, in CTC order
        for r in range(nbest):
            src = perm[b, r]
            assert np.array_equal(res['tokens'][b, r].cpu().numpy(), tokens[b, src])
            assert int(res['len'][b, r]) == out_len[b, src] and float(res['scores'][b, r]) == float(res['total'][b, src])
    assert n_live >= B * 3
    assert total[0, 1] == total[0, 2] and list(perm[0]).index(1) + 1 == list(perm[0]).index(2)      # the exact tie: CTC rank decides


def _load(golden, mode, with_lm):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import TransformerLanguageModel
    g = golden('c1_decode.npz')
    ops.set_compute_dtype(mode)
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    model = ota.SpeechToText(cfg)
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    lm, lm_cfg = None, None
    if with_lm:
        lm_cfg = syn.lm_config(100, d_model=64, d_ff=128, num_blocks=2)
        lm = TransformerLanguageModel(lm_cfg)
        syn.fill_state_dict_(lm.state_dict(), 4321)
        lm = lm.to(DEV).eval()
    return cfg, model.to(DEV).eval(), lm, lm_cfg, torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)


def _rec(model, lm, **kw):
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    return SpeechToTextRecognizer(model, lm=lm, idx2unit={i: str(i) for i in range(100)}, ngpu=1, rescore=True, **kw)


def _head(rec, x, m):
    with torch.no_grad():
        mem, mm, _, _ = rec.encode(x, m)
        lp, ln = rec.model.assistor.inference(mem, mm)
    return mem, mm, lp.float().contiguous(), ln


def _restated(cfg, model, lm, lm_cfg, mem, mm, beam, lam, mu, max_len, penalty, lamda, nbest):
    """the restatement on the oracle's decoder and LM (fp32, CPU) over the model's own encoder memory and the device's own n-best"""
    mem, mm = mem.float().cpu(), mm.cpu()
    sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
    dec = {k[8:]: v for k, v in sd.items() if k.startswith('decoder.')}

    def att_fn(b, h):
        return orc.transformer_decoder(dec, torch.tensor([[EOS] + list(h)]), mem[b:b + 1], mm[b:b + 1], cfg['decoder'])[0].double().numpy()
    lm_fn = None
    if lm is not None:
        lsd = {k: v.float().cpu() for k, v in lm.state_dict().items()}

        def lm_fn(b, h):
            p = torch.tensor([[EOS] + list(h)])
            return torch.stack([orc.lm_step_log_probs((lsd, lm_cfg), p[:, :i + 1])[0] for i in range(p.size(1))]).double().numpy()
    return ref.rescore(beam, att_fn, lam, max_len, lm_fn=lm_fn, mu=mu, penalty=penalty, lamda=lamda, nbest=nbest)


def _tok(nbest):
    return [[tuple(int(t) for t in s.split()) for s in utt] for utt in nbest]


def _cut(h):
    """a hypothesis as nbest_translate prints it: up to the first EOS (the CTC head may emit id 1 like any other token)"""
    return tuple(h[:h.index(EOS)]) if EOS in h else tuple(h)


def _arr(res):
    tok, n = res['tokens'].cpu().numpy(), res['len'].cpu().numpy()
    return [[tuple(int(t) for t in tok[b, r, :n[b, r]]) for r in range(tok.shape[1])] for b in range(tok.shape[0])]


def _close_totals(tot, eps=1e-4):
    live = sorted(t for t in tot if t > -math.inf)
    return any(b - a <= eps for a, b in zip(live, live[1:]))


@pytest.mark.parametrize('with_lm', [False, True])
def test_rescore_end_to_end_fp32(golden, with_lm):
    """fp32 mode on the trained C1 model: tokens identical to the restatement, scores within rtol 1e-5 / atol 1e-4 (the bar of
    test_joint_search_matches_restatement_fp32); an utterance is left out of the token comparison only when two of its restatement
    totals lie within 1e-4, at most 1 of the 4"""
    from opentransformer_amd import ops
    try:
        cfg, model, lm, lm_cfg, x, m = _load(golden, 'fp32', with_lm)
        for lam in (0.3, 0.7):
            kw = dict(beam_width=5, nbest=3, max_len=12, lm_weight=0.3, ctc_weight=lam, penalty=0.6, lamda=5, cutoff_top_n=40)
            rec = _rec(model, lm, **kw)
            mem, mm, lp, ln = _head(rec, x, m)
            res = rec.rescore_pass(mem, mm, lp, ln)
            beam = ref.beam_of(*(t.cpu().numpy() for t in res['beam']))
            want = _restated(cfg, model, lm, lm_cfg, mem, mm, beam, lam, 0.3 if with_lm else 0.0, 12, 0.6, 5.0, 3)
            hyps, scores = rec.recognize(x, m)
            assert torch.equal(scores, res['scores'].cpu())
            got, got_arr = _tok(hyps), _arr(res)
            left_out = 0
            for b in range(4):
                assert any(len(h) > 0 for h, _ in beam[b])                    # a trained model: not degenerate
                print('rescore fp32 lm=%s lam=%.1f utt %d totals %s got %s' % (with_lm, lam, b, want[b]['total'], scores[b].tolist()))
                np.testing.assert_allclose(res['total'][b].cpu().numpy(), np.array(want[b]['total']), rtol=1e-5, atol=1e-4)
                if _close_totals(want[b]['total']):
                    left_out += 1
                    continue
                assert got_arr[b] == want[b]['hyps'], (lam, b)
                assert got[b] == [_cut(h) for h in want[b]['hyps']], (lam, b)
                np.testing.assert_allclose(scores[b].numpy(), np.array(want[b]['scores']), rtol=1e-5, atol=1e-4)
            assert left_out <= 1, left_out
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['bf16', 'fp16'])
def test_rescore_16bit_by_margin(golden, mode):
    """where the fp32 restatement's best and second totals are more than 0.1 apart the 16-bit 1-best is the same and its score within
    5e-2 (as test_joint_cached_matches_reforward_16bit judges); at least 2 utterances are that clear"""
    from opentransformer_amd import ops
    try:
        kw = dict(beam_width=5, nbest=2, max_len=12, lm_weight=0.3, ctc_weight=0.3, cutoff_top_n=40)
        cfg, model, lm, lm_cfg, x, m = _load(golden, 'fp32', True)
        rec = _rec(model, lm, **kw)
        mem, mm, lp, ln = _head(rec, x, m)
        beam = ref.beam_of(*(t.cpu().numpy() for t in rec.rescore_pass(mem, mm, lp, ln)['beam']))
        want = _restated(cfg, model, lm, lm_cfg, mem, mm, beam, 0.3, 0.3, 12, 0.0, 5.0, 2)
        _, model, lm, _, x, m = _load(golden, mode, True)
        rec16 = _rec(model, lm, **kw)
        res16 = rec16.rescore_pass(*_head(rec16, x, m))
        got, scores = _arr(res16), res16['scores'].cpu()
        clear = 0
        for b in range(4):
            s = want[b]['scores']
            print('rescore', mode, 'utt', b, 'want', s, 'got', scores[b].tolist())
            if s[0] - s[1] > 0.1:
                clear += 1
                assert got[b][0] == want[b]['hyps'][0], b
                assert abs(float(scores[b, 0]) - s[0]) < 5e-2, (b, float(scores[b, 0]), s[0])
        assert clear >= 2, clear
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp16', 'bf16'])
def test_shared_memory_fused_route(mode):
    """the fused decoder with ONE set of cross-attention keys / values per utterance (otr_dec_cross_fwd_shared) against the same model
    with the memory repeated W times through the existing launches: the agreement tests/test_gpu_decoder_fused.py asks of fused
    against per-operator (it is in fact the same arithmetic on the same values)"""
    from opentransformer_amd import ops
    from tests.test_gpu_decoder_fused import make_decoder, inputs, rel, row_rel
    ops.set_compute_dtype(mode)
    try:
        vocab, Bm, W = 150, 3, 5
        for Lq, T in ((20, 70), (32, 33), (7, 249)):
            dec = make_decoder(2, 1024, vocab, 0.1, seed=Lq).eval()
            tokens, _, _, _ = inputs(Bm * W, Lq, T, vocab, seed=3)
            _, memory, key_mask, _ = inputs(Bm, Lq, T, vocab, seed=4)
            seen = []
            real = ops.decoder_stack

            def spy(*a, **k):
                seen.append(a[5] if len(a) > 5 else k.get('share', 1))
                return real(*a, **k)
            ops.decoder_stack = spy
            try:
                with torch.no_grad():
                    mem = ops.attach_lp(memory, memory.to(ops.act_dtype()))
                    out = lambda h: ops.linear(h, dec.output_layer.weight, dec.output_layer.bias)    # noqa: E731
                    a = out(dec.hidden(tokens, mem, key_mask, share=W))
                    memr = memory.repeat_interleave(W, dim=0)
                    b, _ = dec(tokens, ops.attach_lp(memr, memr.to(ops.act_dtype())), key_mask.repeat_interleave(W, dim=0))
                    ops._DEC_FUSED = False
                    try:
                        c = out(dec.hidden(tokens, mem, key_mask, share=W))  # not served: per-operator layers on the repeated memory
                    finally:
                        ops._DEC_FUSED = True
            finally:
                ops.decoder_stack = real
            assert seen == [W, 1], seen                                       # the shared launch ran, then the existing one
            assert rel(a, b) < 3e-3 and row_rel(a, b) < 2e-2, (rel(a, b), row_rel(a, b))
            assert torch.equal(a, b)
            assert rel(a, c) < 3e-3 and row_rel(a, c) < 2e-2, (rel(a, c), row_rel(a, c))
    finally:
        ops.set_compute_dtype('bf16')


def test_rescore_takes_the_fused_route_in_16bit():
    """rescore=True on a model of the fused shapes (d_model 256, 4 heads, GLU, post-norm, max_len <= 32) runs the shared launch and
    agrees with the same recognizer on the per-operator route by margin"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ops.set_compute_dtype('fp16')
    try:
        cfg = syn.c2_model(0.0, ctc_weight=0.3)
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 1234)
        model = model.to(DEV).eval()
        V = model.decoder.output_layer.weight.shape[0]
        inputs, _ = syn.synthetic_batch(2, 64, 80, V, 6, seed=3)       # T' = 15 frames: every hypothesis fits max_len
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        from opentransformer_amd.recognize import SpeechToTextRecognizer
        rec = SpeechToTextRecognizer(model, idx2unit={i: str(i) for i in range(V)}, rescore=True, beam_width=4, nbest=2, max_len=32,
                                     ctc_weight=0.5)
        seen = []
        real = ops.decoder_stack

        def spy(*a, **k):
            seen.append(a[5] if len(a) > 5 else k.get('share', 1))
            return real(*a, **k)
        ops.decoder_stack = spy
        try:
            mem, mm, lp, ln = _head(rec, x, m)
            r1 = rec.rescore_pass(mem, mm, lp, ln)
        finally:
            ops.decoder_stack = real
        assert seen == [4], seen
        ops._DEC_FUSED = False
        try:
            r2 = rec.rescore_pass(mem, mm, lp, ln)
        finally:
            ops._DEC_FUSED = True
        t1, t2 = r1['total'].cpu(), r2['total'].cpu()
        live = torch.isfinite(t2)
        assert live.any() and torch.equal(torch.isfinite(t1), live)
        # the two routes' logits agree to 3e-3 relative (tests/test_gpu_decoder_fused.py); a total is a sum of <= 16 log-probs of an
        # untrained model (about -8 each): 5e-2 per 10 units of |total| is that agreement with a margin of about two
        assert float((t1[live] - t2[live]).abs().max()) < 5e-2 * max(1.0, float(t2[live].abs().max()) / 10)
    finally:
        ops.set_compute_dtype('bf16')


def test_graph_capture_replays_identically(golden):
    """search + second pass captured into ONE graph and replayed = eager, also after the log-probs buffer is refilled"""
    from opentransformer_amd import ops
    try:
        _, model, lm, _, x, m = _load(golden, 'fp32', True)
        rec = _rec(model, lm, beam_width=5, nbest=3, max_len=12, lm_weight=0.3, ctc_weight=0.3, penalty=0.6)
        mem, mm, lp1, ln = _head(rec, x, m)
        lp2 = torch.roll(lp1, 1, dims=0).contiguous()
        buf = lp1.clone()
        keys = ('tokens', 'len', 'scores', 'perm', 'total', 'att', 'lm')
        eager1 = {k: rec.rescore_pass(mem, mm, buf, ln)[k].clone() for k in keys}
        buf.copy_(lp2)
        eager2 = {k: rec.rescore_pass(mem, mm, buf, ln)[k].clone() for k in keys}
        assert not torch.equal(eager1['tokens'], eager2['tokens'])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            out = rec.rescore_pass(mem, mm, buf, ln)
        for lp, want in ((lp1, eager1), (lp2, eager2), (lp1, eager1)):
            buf.copy_(lp)
            g.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(out[k], want[k]), k
    finally:
        ops.set_compute_dtype('bf16')


def test_recurrent_lm_is_scored_from_the_zero_state(golden):
    """a RecurrentLanguageModel enters the rescoring as it enters the beam search's shallow fusion (oracle.lm_step_log_probs: the last
    token, no carried state)"""
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import LanguageModel
    try:
        cfg, model, _, _, x, m = _load(golden, 'fp32', False)
        lm_cfg = syn.rnn_lm_config(100, hidden_size=64, num_layers=2)
        lm = LanguageModel['rnn_lm'](lm_cfg)
        syn.fill_state_dict_(lm.state_dict(), 4321)
        lm = lm.to(DEV).eval()
        rec = _rec(model, lm, beam_width=4, nbest=2, max_len=12, lm_weight=0.3, ctc_weight=0.3)
        mem, mm, lp, ln = _head(rec, x, m)
        res = rec.rescore_pass(mem, mm, lp, ln)
        beam = ref.beam_of(*(t.cpu().numpy() for t in res['beam']))
        want = _restated(cfg, model, lm, lm_cfg, mem, mm, beam, 0.3, 0.3, 12, 0.0, 5.0, 2)
        for b in range(4):
            np.testing.assert_allclose(res['total'][b].cpu().numpy(), np.array(want[b]['total']), rtol=1e-5, atol=1e-4)
    finally:
        ops.set_compute_dtype('bf16')


def cross_fwd_case(lib):
    """one seeded otr_dec_cross_fwd problem (fp16 build: 3 utterances x 7 decoder rows in one 32-row group, 45 keys with ragged masks,
    keys / values at columns 0 / 256 of a 512-wide memory) through `lib`'s entry; returns its four outputs as raw bits"""
    import ctypes as C
    from opentransformer_amd import ops
    g = torch.Generator().manual_seed(2024)
    B, Lq, T = 3, 7, 45
    R = B * Lq
    wq, wo = (torch.randn(256, 256, generator=g) / 16).to(DEV), (torch.randn(256, 256, generator=g) / 16).to(DEV)
    bq = (torch.randn(256, generator=g) * 0.1).to(DEV)
    x16 = torch.randn(R, 256, generator=g).to(DEV).half()
    kv = torch.randn(B, T, 512, generator=g).to(DEV).half()
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor([45, 33, 7]).unsqueeze(1)).to(torch.uint8).to(DEV)
    pq, po = ops.lin_packs(wq)[0], ops.lin_packs(wo)[0]
    q16, ctx16 = torch.zeros(R, 256, dtype=torch.half, device=DEV), torch.zeros(R, 256, dtype=torch.half, device=DEV)
    lse, slabs = torch.zeros(B, 4, Lq, device=DEV), torch.zeros(4, R, 256, dtype=torch.half, device=DEV)
    ln = ops._dec_ln(None, x16, None, 0)
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    rc = lib.otr_dec_cross_fwd(C.byref(ln), B, Lq, p(pq), p(bq), p(po), p(kv), T * 512, 512, 0, 256, p(mask), T, p(q16), p(ctx16), p(lse),
                               p(slabs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return {'q16': q16.view(torch.int16).cpu().numpy(), 'ctx16': ctx16.view(torch.int16).cpu().numpy(),
            'lse': lse.view(torch.int32).cpu().numpy(), 'slabs': slabs.view(torch.int16).cpu().numpy()}


def test_existing_cross_attention_launch_is_bit_identical_to_its_record(golden):
    """otr_dec_cross_fwd, whose kernel now shares its body with otr_dec_cross_fwd_shared, still writes the bits it wrote before that
    entry existed: tests/golden/dec_cross_fwd_fp16.npz holds the outputs of the library built from the commit before, on this case"""
    from opentransformer_amd import _lib, ops
    ops.set_compute_dtype('fp16')
    try:
        got, want = cross_fwd_case(_lib.load()), golden('dec_cross_fwd_fp16.npz')
        for k in ('q16', 'ctx16', 'lse', 'slabs'):
            assert np.array_equal(got[k], want[k]), k
        assert np.abs(got['slabs'].astype(np.int32)).max() > 0
    finally:
        ops.set_compute_dtype('bf16')
