"""GPU (-m gpu): decode parity -- token-identical greedy / beam / LM-fusion hypotheses and scores
against the fixtures the REAL reference recognizers produced on a briefly trained C1 model
(tests/golden/c1_decode.npz, oracle/make_golden.py:golden_decode)."""
import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def load_models(g, mode):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import TransformerLanguageModel
    ops.set_compute_dtype(mode)
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    lm = TransformerLanguageModel(syn.lm_config(100, d_model=64, d_ff=128, num_blocks=2))
    syn.fill_state_dict_(lm.state_dict(), 4321)
    return model.to(DEV).eval(), lm.to(DEV).eval()


def hyp_arr(nbest, like):
    a = -np.ones_like(like)
    for i, utt in enumerate(nbest):
        for j, s in enumerate(utt):
            toks = [int(t) for t in s.split()]
            a[i, j, :len(toks)] = toks
    return a


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'fp16'])
def test_beam_search_matches_reference(golden, mode):
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    g = golden('c1_decode.npz')
    try:
        model, lm = load_models(g, mode)
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        idx2unit = {i: str(i) for i in range(100)}
        for tag, kw in [('greedy', dict(beam_width=1, nbest=1, max_len=12, penalty=0.0)),
                        ('beam5', dict(beam_width=5, nbest=5, max_len=12, penalty=0.6, lamda=5)),
                        ('beam5_lm', dict(beam_width=5, nbest=3, max_len=12, penalty=0.6, lamda=5, lm=lm, lm_weight=0.3))]:
            rec = SpeechToTextRecognizer(model, idx2unit=idx2unit, ngpu=1, **kw)
            nbest, scores = rec.recognize(x, m)
            want = g[tag + '_hyp']
            got = hyp_arr(nbest, want)
            if mode == 'fp32':
                assert np.array_equal(got, want), tag
                np.testing.assert_allclose(scores.numpy(), g[tag + '_score'], rtol=2e-4, atol=2e-4)
            else:
                # bf16: the 1-best must be token-identical wherever the REFERENCE's own 1-best/2-best
                # score margin exceeds 0.1 nat; below that bf16 rounding may legitimately swap beams
                # (one such utterance exists: LM-fused scores -12.427 / -12.477 / -12.551).
                ref_s = g[tag + '_score']
                clear = np.ones(len(want), bool) if ref_s.shape[1] < 2 else (ref_s[:, 0] - ref_s[:, 1]) > 0.1
                assert clear.sum() >= 3, tag
                assert np.array_equal(got[clear, 0], want[clear, 0]), tag
                np.testing.assert_allclose(scores.numpy()[clear, 0], ref_s[clear, 0], rtol=5e-2, atol=5e-2)
    finally:
        ops.set_compute_dtype('bf16')


def test_decoder_inference_lm_and_ctc_greedy_match_reference(golden):
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import CTCRecognizer
    g = golden('c1_decode.npz')
    try:
        model, lm = load_models(g, 'fp32')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        with torch.no_grad():
            fe, fm, _ = model.frontend.inference(x, m, None)
            mem, mm, _ = model.encoder(fe, fm)
            preds = torch.from_numpy(g['inference_preds']).to(DEV)
            lp, _, _ = model.decoder.inference(preds, mem, mm)
            np.testing.assert_allclose(lp.cpu().numpy(), g['inference_logp'], rtol=1e-4, atol=1e-4)
            llp = lm.predict(preds, last_frame=True).squeeze(1)
            np.testing.assert_allclose(llp.cpu().numpy(), g['lm_logp'], rtol=1e-4, atol=1e-4)
            clp, cln = model.assistor.inference(mem, mm)
            np.testing.assert_allclose(clp.cpu().numpy(), g['ctc_head_logp'], rtol=1e-4, atol=2e-4)
        greedy = CTCRecognizer(model, idx2unit={i: str(i) for i in range(100)}, mode='greedy').recognize_greedy(x, m)
        want = [[t for t in row if t >= 0] for row in g['ctc_greedy'].tolist()]
        assert greedy == want
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_recurrent_lm_and_its_shallow_fusion_match_reference(golden, mode):
    """model/lm.py:33-91 + recognize/base.py:26-37 against the fixture the REAL reference produced (tests/golden/c1_decode_rnnlm.npz,
    oracle/make_golden.py:golden_decode_rnnlm): RecurrentLanguageModel.predict from zeros and from a carried state, and the beam
    search fused with it -- re-forward loop, KV-cached eager and KV-cached under hipGraph replay all give the reference's n-best."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import LanguageModel, SpeechToTextRecognizer
    g, base = golden('c1_decode_rnnlm.npz'), golden('c1_decode.npz')
    ops.set_compute_dtype(mode)
    try:
        model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
        model.load_state_dict({k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith('w:')}, strict=True)
        model = model.to(DEV).eval()
        lm = LanguageModel['rnn_lm'](syn.rnn_lm_config(100, hidden_size=64, num_layers=2))
        syn.fill_state_dict_(lm.state_dict(), 4321)
        lm = lm.to(DEV).eval()
        tol = dict(rtol=1e-4, atol=1e-4) if mode == 'fp32' else dict(rtol=3e-2, atol=3e-2)
        toks = torch.from_numpy(g['predict_tokens']).to(DEV)
        lp, (h, c) = lm.predict(toks)
        np.testing.assert_allclose(lp.cpu().numpy(), g['predict_logp'], **tol)
        np.testing.assert_allclose(h.cpu().numpy(), g['predict_h'], **tol)
        np.testing.assert_allclose(c.cpu().numpy(), g['predict_c'], **tol)
        lp2, (h2, c2) = lm.predict(toks[:, :2], (h, c))
        np.testing.assert_allclose(lp2.cpu().numpy(), g['predict2_logp'], **tol)
        np.testing.assert_allclose(c2.cpu().numpy(), g['predict2_c'], **tol)
        x, m = torch.from_numpy(base['inputs']).to(DEV), torch.from_numpy(base['mask']).to(DEV)
        want, ref_s = g['beam5_rnnlm_hyp'], g['beam5_rnnlm_score']
        for cache, graph in ((False, False), (True, False), (True, True)):
            rec = SpeechToTextRecognizer(model, idx2unit={i: str(i) for i in range(100)}, ngpu=1, beam_width=5, nbest=3, max_len=12, penalty=0.6,
                                         lamda=5, lm=lm, lm_weight=0.3, apply_cache=cache)
            rec.use_hipgraph = graph
            for _ in range(2 if graph else 1):          # the second call replays the captured step graphs
                nbest, scores = rec.recognize(x, m)
            got = hyp_arr(nbest, want)
            if mode == 'fp32':
                assert np.array_equal(got, want), (cache, graph)
                np.testing.assert_allclose(scores.numpy(), ref_s, rtol=2e-4, atol=2e-4)
            else:
                clear = (ref_s[:, 0] - ref_s[:, 1]) > 0.1     # the reference's own 1-best / 2-best margin (as test_beam_search_matches_reference)
                assert clear.sum() >= 2
                assert np.array_equal(got[clear, 0], want[clear, 0]), (cache, graph)
                np.testing.assert_allclose(scores.numpy()[clear, 0], ref_s[clear, 0], rtol=5e-2, atol=5e-2)
    finally:
        ops.set_compute_dtype('bf16')


def test_beam_kernels_against_torch():
    """otr_beam_topk / otr_beam_prune vs the reference's own torch formulation on random scores."""
    import ctypes as C
    from opentransformer_amd import _lib as L
    from oracle import otrans_oracle as orc     # noqa: F401  (semantics documented there)
    lib = L.load()
    gen = torch.Generator().manual_seed(0)
    R, V, k = 12, 4234, 5
    logits = torch.randn(R, 3, V, generator=gen).to(DEV)
    lm = torch.randn(R, 3, V, generator=gen).to(DEV)
    ks = torch.empty(R, k, device=DEV)
    ki = torch.empty(R, k, dtype=torch.long, device=DEV)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off * t.element_size())      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.otr_beam_topk(p(logits, 2 * V), 3 * V, p(lm, 2 * V), 3 * V, 0.3, R, V, k, p(ks), p(ki), st), 'topk')
    ref = torch.log_softmax(logits[:, -1], -1) + 0.3 * torch.log_softmax(lm[:, -1], -1)
    rs, ri = ref.topk(k)
    assert torch.equal(ki, ri)
    torch.testing.assert_close(ks, rs, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------------- KV-cached decoding (8f rank 1)
DECODE_CASES = [('greedy', dict(beam_width=1, nbest=1, max_len=12, penalty=0.0), False),
                ('beam5', dict(beam_width=5, nbest=5, max_len=12, penalty=0.6, lamda=5), False),
                ('beam5_lm', dict(beam_width=5, nbest=3, max_len=12, penalty=0.6, lamda=5, lm_weight=0.3), True)]


def test_cached_beam_search_matches_reference_fp32(golden):
    """apply_cache=True (one token per step, hipGraph replay) must reproduce the reference recognizer's
    hypotheses and scores; eager-cached, graph-cached and a re-run on the warmed state all agree."""
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    g = golden('c1_decode.npz')
    try:
        model, lm = load_models(g, 'fp32')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        idx2unit = {i: str(i) for i in range(100)}
        for tag, kw, use_lm in DECODE_CASES:
            kw = dict(kw, lm=lm) if use_lm else kw
            want = g[tag + '_hyp']
            for graph in (False, True):
                rec = SpeechToTextRecognizer(model, idx2unit=idx2unit, ngpu=1, apply_cache=True, **kw)
                rec.use_hipgraph = graph
                for rerun in range(3 if graph else 1):          # re-runs replay the captured graphs from step 1
                    nbest, scores = rec.recognize(x, m)
                    assert np.array_equal(hyp_arr(nbest, want), want), (tag, graph, rerun)
                    np.testing.assert_allclose(scores.numpy(), g[tag + '_score'], rtol=2e-4, atol=2e-4)
                if graph:
                    st = next(iter(rec._cached_states.values()))
                    assert st.graphs[0] is not None and st.graphs[1] is not None
    finally:
        ops.set_compute_dtype('bf16')


def test_cached_beam_search_bf16_matches_uncached(golden):
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    g = golden('c1_decode.npz')
    try:
        model, lm = load_models(g, 'bf16')
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        idx2unit = {i: str(i) for i in range(100)}
        for tag, kw, use_lm in DECODE_CASES:
            kw = dict(kw, lm=lm) if use_lm else kw
            want = g[tag + '_hyp']
            ref_s = g[tag + '_score']
            nbest, scores = SpeechToTextRecognizer(model, idx2unit=idx2unit, apply_cache=True, **kw).recognize(x, m)
            clear = np.ones(len(want), bool) if ref_s.shape[1] < 2 else (ref_s[:, 0] - ref_s[:, 1]) > 0.1
            assert np.array_equal(hyp_arr(nbest, want)[clear, 0], want[clear, 0]), tag
            np.testing.assert_allclose(scores.numpy()[clear, 0], ref_s[clear, 0], rtol=5e-2, atol=5e-2)
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'fp16'])
def test_cached_decode_full_size_c5(mode):
    """C5 shape (transformer_baseline dims, beam 10, 4-block LM fusion, V=4234): with EOS suppressed so every
    hypothesis runs the full max_len, the cached loop and the reference-style re-forward loop agree."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer, TransformerLanguageModel
    ops.set_compute_dtype(mode)
    try:
        cfg = syn.c2_model(0.0, n_enc=2)
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 7)
        lm = TransformerLanguageModel(syn.lm_config(4234, num_blocks=2))
        syn.fill_state_dict_(lm.state_dict(), 8)
        with torch.no_grad():
            model.decoder.output_layer.bias[1] = -30.0          # EOS never wins: decode runs max_len steps
        model, lm = model.to(DEV).eval(), lm.to(DEV).eval()
        inputs, _ = syn.synthetic_batch(batch=3, frames=400, feat_dim=80, vocab=4234, tgt_len=5, seed=3,
                                        lengths=[400, 333, 250])
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        idx2unit = {i: str(i) for i in range(4234)}
        kw = dict(beam_width=10, nbest=10, max_len=16, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, idx2unit=idx2unit)
        ref_h, ref_s = SpeechToTextRecognizer(model, apply_cache=False, **kw).recognize(x, m)
        rec = SpeechToTextRecognizer(model, apply_cache=True, **kw)
        for _ in range(2):
            got_h, got_s = rec.recognize(x, m)
            if mode == 'fp32':
                assert got_h == ref_h
                np.testing.assert_allclose(got_s.numpy(), ref_s.numpy(), rtol=1e-4, atol=1e-4)
            else:
                assert [h[0] for h in got_h] == [h[0] for h in ref_h] or \
                    np.allclose(got_s.numpy()[:, 0], ref_s.numpy()[:, 0], rtol=2e-2, atol=5e-2)
                np.testing.assert_allclose(got_s.numpy()[:, 0], ref_s.numpy()[:, 0], rtol=2e-2, atol=5e-2)
        assert all(len(h[0].split()) == 16 for h in got_h)
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('variant', [(True, False), (False, True), (True, True)])
def test_cached_decode_layer_variants(variant):
    """pre-norm / concat_after decoders: the cached one-token step agrees with the re-forward loop, which itself runs the
    training forward that tests/test_gpu_model.py pins against the reference fixture."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    ops.set_compute_dtype('fp32')
    try:
        model = ota.SpeechToText(syn.c1_variant(*variant, ctc_weight=0.0))
        syn.fill_state_dict_(model.state_dict(), 17)
        with torch.no_grad():
            model.decoder.output_layer.bias[1] = -30.0          # EOS never wins: decode runs max_len steps
        model = model.to(DEV).eval()
        inputs, _ = syn.synthetic_batch(batch=3, frames=160, feat_dim=80, vocab=100, tgt_len=5, seed=4, lengths=[160, 121, 90])
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        kw = dict(beam_width=4, nbest=4, max_len=9, penalty=0.6, lamda=5, idx2unit={i: str(i) for i in range(100)})
        ref_h, ref_s = SpeechToTextRecognizer(model, apply_cache=False, **kw).recognize(x, m)
        rec = SpeechToTextRecognizer(model, apply_cache=True, **kw)
        for _ in range(2):
            got_h, got_s = rec.recognize(x, m)
            assert got_h == ref_h
            np.testing.assert_allclose(got_s.numpy(), ref_s.numpy(), rtol=1e-4, atol=1e-4)
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_decode_self_attention_kernel(dtype):
    """One new query per hypothesis against a tree-structured cache (ancestor table), positions beyond one
    64-lane chunk, vs a dense torch reference that gathers each hypothesis' ancestor rows."""
    from opentransformer_amd import ops
    gen = torch.Generator().manual_seed(5)
    R, H, dk, maxlen, p = 7, 4, 24, 150, 133
    d = H * dk
    qkv = torch.randn(R, 3 * d, generator=gen).to(DEV, dtype)
    kc = torch.randn(R, maxlen, d, generator=gen).to(DEV, dtype)
    vc = torch.randn(R, maxlen, d, generator=gen).to(DEV, dtype)
    anc = torch.randint(0, R, (R, maxlen), generator=gen).to(DEV, torch.int32)
    pos = torch.tensor([p], dtype=torch.int32, device=DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    out = ops.decode_self_attention(qkv, kc, vc, anc, pos, H).float()
    q, kn, vn = [t.float() for t in qkv.split(d, dim=-1)]
    rows = anc[:, :p].long()                                                    # [R,p]
    K = torch.cat([kc0.float()[rows, torch.arange(p, device=DEV)], kn[:, None]], 1)      # [R,p+1,d]
    Vv = torch.cat([vc0.float()[rows, torch.arange(p, device=DEV)], vn[:, None]], 1)
    s = torch.einsum('rhd,rjhd->rhj', q.view(R, H, dk), K.view(R, p + 1, H, dk)) / dk ** 0.5
    ref = torch.einsum('rhj,rjhd->rhd', s.softmax(-1), Vv.view(R, p + 1, H, dk)).reshape(R, d)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(out, ref, rtol=tol, atol=tol)
    # the new k/v were stored at position p of the hypothesis' own row, everything else untouched
    assert torch.equal(kc[:, p], qkv[:, d:2 * d]) and torch.equal(vc[:, p], qkv[:, 2 * d:])
    kc[:, p], vc[:, p] = kc0[:, p], vc0[:, p]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


def test_decode_embed_and_prune_cached_kernels():
    import ctypes as C
    from opentransformer_amd import _lib as L
    from opentransformer_amd import ops
    lib = L.load()
    gen = torch.Generator().manual_seed(9)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # embed at a device-side position == column `pos` of the full embed+posenc
    R, ldp, V, d, pos_i = 6, 9, 50, 32, 4
    preds = torch.randint(0, V, (R, ldp), generator=gen).to(DEV)
    E = torch.randn(V, d, generator=gen).to(DEV)
    pos = torch.tensor([pos_i], dtype=torch.int32, device=DEV)
    full = ops.embed_posenc(preds, E)
    one = ops.decode_embed(preds, pos, E)
    assert torch.equal(one, full[:, pos_i])
    # prune_cached == prune (+ ancestor re-parenting, + position increment)
    batch, beam, t = 3, 4, 5
    Rb, ldp, maxlen = batch * beam, 12, 11
    ks = torch.randn(Rb, beam, generator=gen).to(DEV)
    ki = torch.randint(0, 30, (Rb, beam), generator=gen).to(DEV)
    ki[2, 0] = 1
    sc = torch.randn(Rb, generator=gen).to(DEV)
    fl = (torch.rand(Rb, generator=gen) < 0.3).to(DEV, torch.uint8)
    pr = torch.randint(2, 30, (Rb, ldp), generator=gen).to(DEV)
    anc = torch.randint(0, Rb, (Rb, maxlen), generator=gen).to(DEV, torch.int32)
    o = dict(s=torch.empty_like(sc), f=torch.empty_like(fl), p=torch.zeros_like(pr), n=torch.zeros(1, dtype=torch.int32, device=DEV))
    L.check(lib.otr_beam_prune(p(ks), p(ki), p(sc), p(fl), p(pr), ldp, batch, beam, t, 1, p(o['s']), p(o['f']), p(o['p']),
                               p(o['n']), st), 'prune')
    c = dict(s=torch.empty_like(sc), f=torch.empty_like(fl), p=torch.zeros_like(pr), n=torch.zeros(2, dtype=torch.int32, device=DEV))
    pin = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
    pout = torch.zeros(1, dtype=torch.int32, device=DEV)
    anc2 = torch.full_like(anc, -1)
    L.check(lib.otr_beam_prune_cached(p(ks), p(ki), p(sc), p(fl), p(pr), ldp, batch, beam, 1, p(pin), p(pout), p(anc), p(anc2),
                                      maxlen, p(c['s']), p(c['f']), p(c['p']), p(c['n']), st), 'prune_cached')
    for rep in range(2):                 # the arrival word resets itself: a second launch on the same buffer counts from zero again
        for k in o:
            assert torch.equal(o[k], c[k][:o[k].shape[0]] if k == 'n' else c[k]), k
        assert int(c['n'][1]) == 0
        if rep == 0:
            L.check(lib.otr_beam_prune_cached(p(ks), p(ki), p(sc), p(fl), p(pr), ldp, batch, beam, 1, p(pin), p(pout), p(anc), p(anc2),
                                              maxlen, p(c['s']), p(c['f']), p(c['p']), p(c['n']), st), 'prune_cached')
    assert int(pout) == t
    # parent of each surviving hypothesis = the row whose prefix it inherited
    for r in range(Rb):
        u = r // beam
        parents = [q for q in range(u * beam, (u + 1) * beam) if torch.equal(pr[q, :t], c['p'][r, :t])]
        par = int(anc2[r, t - 1])
        assert par in parents
        assert torch.equal(anc2[r, :t - 1], anc[par, :t - 1])
        assert bool((anc2[r, t:] == -1).all())


@pytest.mark.parametrize('mode', ['fp16', 'bf16'])
def test_cached_search_fused_step_matches_unfused_step(mode):
    """the cached beam search at the C5 shapes on otr_dec_self_step + the fused tail vs the same search on the per-operator launches
    (qkv GEMM, otr_decode_self_attention, output projection + LayerNorm): same hypotheses wherever the margin is clear, close scores"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops, recognize, synthetic as syn
    ops.set_compute_dtype(mode)
    try:
        model = ota.SpeechToText(syn.c2_model(0.0, n_enc=2))
        syn.fill_state_dict_(model.state_dict(), 7)
        lm = recognize.TransformerLanguageModel(syn.lm_config(4234, num_blocks=2))
        syn.fill_state_dict_(lm.state_dict(), 8)
        with torch.no_grad():
            model.decoder.output_layer.bias[1] = -30.0          # EOS never wins: every hypothesis runs max_len steps
        model, lm = model.to(DEV).eval(), lm.to(DEV).eval()
        inputs, _ = syn.synthetic_batch(batch=3, frames=400, feat_dim=80, vocab=4234, tgt_len=5, seed=3, lengths=[400, 333, 250])
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        kw = dict(beam_width=10, nbest=10, max_len=20, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, idx2unit={i: str(i) for i in range(4234)})
        res = {}
        for fused in (True, False):
            recognize._DECODE_STEP_FUSED = fused
            rec = recognize.SpeechToTextRecognizer(model, apply_cache=True, **kw)
            res[fused] = rec.recognize(x, m)
            stt = next(iter(rec._cached_states.values()))
            assert stt.fused_dec == fused and stt.fused_lm == fused
        (h1, s1), (h0, s0) = res[True], res[False]
        s1, s0 = s1.numpy(), s0.numpy()
        tol = 0.15 if mode == 'bf16' else 0.03
        assert abs(s1[:, 0] - s0[:, 0]).max() < tol, (s1[:, 0], s0[:, 0])
        for i in range(len(h0)):
            if s0[i, 0] - s0[i, 1] > 2 * tol:
                assert h1[i][0] == h0[i][0], i
    finally:
        recognize._DECODE_STEP_FUSED = True
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp16', 'bf16'])
@pytest.mark.parametrize('lm_blocks,dec_blocks', [(2, 3), (4, 2), (3, 3)])
def test_cached_search_on_pair_launches_is_the_forked_search(mode, lm_blocks, dec_blocks):
    """r06: the LM's layers as the second problem of the decoder's launches (otr_dec_self_step_pair / otr_dec_ffn_fwd_pair /
    otr_dec_ln_pair, recognize.CachedBeamState._walk on two chains) run the same kernels on the same operands as the two separate
    chains (the LM on a forked stream): token-identical n-best lists and bit-equal scores, also when one stack is deeper than the other
    (the tail of the deeper one runs on single launches), eagerly and under hipGraph replay."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops, recognize, synthetic as syn
    ops.set_compute_dtype(mode)
    try:
        cfg = syn.c2_model(0.0, n_enc=2)
        cfg['decoder']['n_blocks'] = dec_blocks
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 7)
        lm = recognize.TransformerLanguageModel(syn.lm_config(4234, num_blocks=lm_blocks))
        syn.fill_state_dict_(lm.state_dict(), 8)
        with torch.no_grad():
            model.decoder.output_layer.bias[1] = 2.0            # EOS live: beams finish at different steps
        model, lm = model.to(DEV).eval(), lm.to(DEV).eval()
        inputs, _ = syn.synthetic_batch(batch=3, frames=400, feat_dim=80, vocab=4234, tgt_len=5, seed=3, lengths=[400, 333, 250])
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        kw = dict(beam_width=10, nbest=10, max_len=16, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, idx2unit={i: str(i) for i in range(4234)})
        res = {}
        for pair in (True, False):
            recognize._DECODE_PAIR = pair
            rec = recognize.SpeechToTextRecognizer(model, apply_cache=True, **kw)
            res[pair] = rec.recognize(x, m)
            stt = next(iter(rec._cached_states.values()))
            assert stt.paired == pair and (stt.side is None) == pair
            if pair:
                assert all(g is not None for g in stt.graphs)      # the paired step was captured and replayed
        (h1, s1), (h0, s0) = res[True], res[False]
        assert h1 == h0
        assert torch.equal(s1, s0)
    finally:
        recognize._DECODE_PAIR = True
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp16', 'fp32'])
def test_cached_search_with_the_lagged_stop_test_is_the_synchronous_search(mode):
    """r06 (recognize._DECODE_LAGGED_STOP): the cached beam search launches step s + 1 before it reads step s's all-finished count and
    gives back exactly what the loop that syncs after every step (recognize/speech2text.py:67) gives: hypotheses, scores, and the step
    it stopped at.  With EOS live the search stops early, so the one step that ran in vain is exercised."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops, recognize, synthetic as syn
    ops.set_compute_dtype(mode)
    try:
        cfg = syn.c2_model(0.0, n_enc=2)
        cfg['decoder']['n_blocks'] = 2
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 17)
        lm = recognize.TransformerLanguageModel(syn.lm_config(4234, num_blocks=2))
        syn.fill_state_dict_(lm.state_dict(), 18)
        with torch.no_grad():
            model.decoder.output_layer.bias[1] = 30.0           # EOS wins everywhere: every beam has finished after two or three steps
        model, lm = model.to(DEV).eval(), lm.to(DEV).eval()
        inputs, _ = syn.synthetic_batch(batch=3, frames=400, feat_dim=80, vocab=4234, tgt_len=5, seed=5, lengths=[400, 333, 250])
        x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
        kw = dict(beam_width=10, nbest=10, max_len=24, penalty=0.6, lamda=5, lm=lm, lm_weight=0.1, idx2unit={i: str(i) for i in range(4234)})
        res, stops = {}, {}
        run0 = recognize.CachedBeamState.run

        def run_and_note(self):
            out = run0(self)
            stops.setdefault(recognize._DECODE_LAGGED_STOP, []).append(out[1])
            return out
        recognize.CachedBeamState.run = run_and_note
        for lag in (False, True):
            recognize._DECODE_LAGGED_STOP = lag
            rec = recognize.SpeechToTextRecognizer(model, apply_cache=True, **kw)
            for _ in range(4):                                 # eager warm-up visits, capture, replay
                res[lag] = rec.recognize(x, m)
        assert stops[False] == stops[True] and max(stops[False]) < 24, stops    # the search did stop early, at the same step every time
        assert res[True][0] == res[False][0]
        assert torch.equal(res[True][1], res[False][1])
    finally:
        recognize._DECODE_LAGGED_STOP = True
        recognize.CachedBeamState.run = run0
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('joint,ngram', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('lm_kind', ['none', 'transformer', 'recurrent'])
def test_both_loops_take_the_same_steps_fp32(golden, lm_kind, joint, ngram):
    """the re-forward loop and the cached loop (eager: with `trace` set its run syncs after every step) hand the shared scoring tail
    the same state: after EVERY step the same prefixes and, to the file's fp32 bound of cached against reference, the same cumulative
    scores, and both stop at the same step -- with and without each LM, the joint CTC scores and the n-gram's addend"""
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import LanguageModel, SpeechToTextRecognizer
    from tests import ngram_attn_cases as cs
    g = golden('c1_decode.npz')
    try:
        model, lm = load_models(g, 'fp32')
        if lm_kind == 'recurrent':
            lm = LanguageModel['rnn_lm'](syn.rnn_lm_config(100, hidden_size=64, num_layers=2))
            syn.fill_state_dict_(lm.state_dict(), 4321)
            lm = lm.to(DEV).eval()
        x, m = torch.from_numpy(g['inputs']).to(DEV), torch.from_numpy(g['mask']).to(DEV)
        kw = dict(lm=lm if lm_kind != 'none' else None, lm_weight=0.3, ctc_weight=0.3, beam_width=4, nbest=4, max_len=8, joint_ctc=joint,
                  idx2unit={i: str(i) for i in range(100)})
        if ngram:
            kw.update(ngram_lm=cs.ngram(5)[0], alpha=0.5, beta=1.0)
        traces = {}
        for cache in (False, True):
            rec = SpeechToTextRecognizer(model, apply_cache=cache, **kw)
            rec.use_hipgraph = False
            rec.trace = traces[cache] = []
            rec.recognize(x, m)
        assert len(traces[False]) == len(traces[True]) >= 1, (len(traces[False]), len(traces[True]))
        for step, ((p0, s0), (p1, s1)) in enumerate(zip(traces[False], traces[True]), 1):
            assert p0.shape == (x.size(0) * 4, step + 1)
            assert torch.equal(p0, p1), step
            print(lm_kind, joint, ngram, 'step', step, 'max |d score| %.3g' % float((s0 - s1)[torch.isfinite(s0)].abs().max()))
            torch.testing.assert_close(s1, s0, rtol=2e-4, atol=2e-4, msg=lambda t: 'step %d: %s' % (step, t))
    finally:
        ops.set_compute_dtype('bf16')
