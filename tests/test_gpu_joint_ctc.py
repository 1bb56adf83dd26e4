"""GPU (-m gpu): the joint CTC/attention beam search (SpeechToTextRecognizer joint_ctc=True, csrc/ctcscore.hip) against the
plain-Python restatement (tests/ctc_prefix_score_ref.py) built on the oracle's decoder, CTC head and LM (oracle/otrans_oracle.py)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opentransformer_amd import synthetic as syn
from oracle import otrans_oracle as orc
from tests import ctc_prefix_score_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BLANK, EOS = 0, 1


def peaky(rng, B, T, V):
    lg = rng.normal(size=(B, T, V)) * 4.0
    lg[..., BLANK] += 3.0
    return lg - np.log(np.exp(lg).sum(-1, keepdims=True))


@pytest.mark.parametrize('T', [1, 33, 249, 2048])
def test_prefix_score_kernel_matches_restatement(T):
    """ragged lengths, prefix lengths from 0 to beyond T_b, candidates that include blank, EOS and the last token; the parent state is
    the restatement's.  -inf exactly where the restatement has -inf, |d psi| <= 1e-4 (+ 1e-6 |psi|: f32 sums of hundreds of frames)."""
    from opentransformer_amd import ops
    rng = np.random.default_rng(T)
    B, V, K, rpu = 3, 40, 10, 4
    lens = [T, max(1, T // 2), max(1, T // 5)]
    lp = peaky(rng, B, T, V)
    R = B * rpu
    ldp = 16
    x = [lp[b].tolist() for b in range(B)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    lp_d, len_d = dev(lp.astype(np.float32)), dev(np.array(lens, np.int32))
    n_fin = 0
    for n in (0, 1, 3, 9):                                 # prefix lengths: 9 tokens do not fit the short utterances
        preds = np.full((R, ldp), EOS, np.int64)
        cands = np.zeros((R, K), np.int32)
        rn_in, rb_in, psi_in = np.zeros((R, T), np.float32), np.zeros((R, T), np.float32), np.zeros(R, np.float32)
        want, want_state = [], []
        for r in range(R):
            b = r // rpu
            Tb = lens[b]
            g = [int(v) for v in rng.integers(2, V, size=n)]
            if n >= 2:
                g[-1] = g[-2]                              # a repeat inside the prefix
            preds[r, 1:1 + n] = g
            st = ref.prefix_state(x[b], Tb, g, BLANK, EOS)
            if n >= 1:
                rn_in[r, :Tb], rb_in[r, :Tb], psi_in[r] = st[0], st[1], st[2]
            c = [BLANK, EOS] + ([g[-1]] if n else []) + [int(v) for v in rng.choice(np.arange(2, V), size=K, replace=False)]
            c = list(dict.fromkeys(c))[:K]
            cands[r] = c
            res = [ref.extend(st, x[b], Tb, cc, BLANK, EOS) for cc in c]
            want.append([p for p, _ in res])
            want_state.append([s for _, s in res])
        rn_o = torch.full((R * K, T), 7.0, device=DEV)
        rb_o, psi_o = rn_o.clone(), torch.full((R * K,), 7.0, device=DEV)
        ops.ctc_prefix_score(lp_d, len_d, dev(cands), dev(preds), n + 1, rpu, BLANK, EOS, dev(np.arange(R, dtype=np.int32)),
                             (dev(rn_in), dev(rb_in), dev(psi_in)), (rn_o, rb_o, psi_o))
        torch.cuda.synchronize()
        got = psi_o.view(R, K).cpu().numpy().astype(np.float64)
        w = np.array(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(w)), n
        fin = ~np.isneginf(w)
        n_fin += fin.sum()
        assert np.all(np.abs(got[fin] - w[fin]) <= 1e-4 + 1e-6 * np.abs(w[fin])), (n, np.abs(got[fin] - w[fin]).max())
        # the candidates' states (frames < T_b) where the restatement has one: the same bar relative to f32 sums of up to 2048 frames
        rn_g, rb_g = rn_o.view(R, K, T).cpu().numpy(), rb_o.view(R, K, T).cpu().numpy()
        for r in range(R):
            Tb = lens[r // rpu]
            for k in range(K):
                s = want_state[r][k]
                if s is None:
                    continue
                for a, e in ((rn_g[r, k, :Tb], np.array(s[0])), (rb_g[r, k, :Tb], np.array(s[1]))):
                    assert np.array_equal(np.isneginf(a), np.isneginf(e)), (n, r, k)
                    f = ~np.isneginf(e)
                    assert np.all(np.abs(a[f] - e[f]) <= 1e-4 + 1e-5 * np.abs(e[f])), (n, r, k)
    assert n_fin > 2 * R


def _setup(mode, lm_kind=None, cfg=None, seed=11):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.recognize import LanguageModel
    ops.set_compute_dtype(mode)
    cfg = cfg or syn.c1_model(0.0, ctc_weight=0.3)
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).eval()
    lm, lm_cfg = None, None
    if lm_kind == 'transformer':
        lm_cfg = syn.lm_config(100, d_model=64, d_ff=128, num_blocks=2)
        lm = LanguageModel['transformer_lm'](lm_cfg)
    elif lm_kind == 'rnn':
        lm_cfg = syn.rnn_lm_config(100, hidden_size=64, num_layers=2)
        lm = LanguageModel['rnn_lm'](lm_cfg)
    if lm is not None:
        syn.fill_state_dict_(lm.state_dict(), 4321)
        lm = lm.to(DEV).eval()
    inputs, _ = syn.synthetic_batch(batch=4, frames=120, feat_dim=80, vocab=100, tgt_len=6, seed=seed, lengths=[120, 96, 13, 70],
                                    tgt_lengths=[6, 6, 6, 6])
    return cfg, model, lm, lm_cfg, inputs['inputs'].to(DEV), inputs['mask'].to(DEV)


def _rec(model, lm, **kw):
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    return SpeechToTextRecognizer(model, lm=lm, idx2unit={i: str(i) for i in range(100)}, ngpu=1, **kw)


def _restated(cfg, model, lm, lm_cfg, x, m, beam, max_len, lam, lm_weight, K, nbest):
    """the restatement on the oracle's decoder / CTC head / LM over the model's own encoder memory (fp32)"""
    with torch.no_grad():
        rec = _rec(model, None)
        mem, mm, _, _ = rec.encode(x, m)
    mem, mm = mem.float().cpu(), mm.cpu()
    sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
    dec = {k[8:]: v for k, v in sd.items() if k.startswith('decoder.')}
    ctc = {k[9:]: v for k, v in sd.items() if k.startswith('assistor.')}
    B, T, D = mem.shape
    bm = mem.unsqueeze(1).repeat(1, beam, 1, 1).view(B * beam, T, D)
    bmask = mm.unsqueeze(1).repeat(1, beam, 1).view(B * beam, T)
    att = lambda p: orc.decoder_inference(dec, p, bm, bmask, cfg['decoder'])          # noqa: E731
    lm_fn = None
    if lm is not None:
        lsd = {k: v.float().cpu() for k, v in lm.state_dict().items()}
        lm_fn = lambda p: orc.lm_step_log_probs((lsd, lm_cfg), p)                     # noqa: E731
    clp, cln = orc.ctc_inference(ctc, mem, mm)
    joint = dict(x=clp.double().tolist(), lengths=cln.tolist(), ctc_weight=lam, K=K, blank=BLANK)
    hyps, scores = ref.beam_search(att, B, beam, max_len, EOS, lm_fn=lm_fn, lm_weight=lm_weight, joint=joint, nbest=nbest)
    return hyps, scores, (dec, clp, cln, lm_fn)


def _tok(nbest):
    return [[[int(t) for t in s.split()] for s in utt] for utt in nbest]


@pytest.mark.parametrize('lm_kind', [None, 'transformer'])
def test_joint_search_matches_restatement_fp32(lm_kind):
    """fp32, both loops: identical tokens, scores within 1e-4; utterance 2 (13 frames -> T' = 2) is ended early by the CTC head.
    And the telescoped sum: every returned 1-best that ended in EOS scores (1-lambda) log P_att + lambda log P_ctc + lm_weight log P_lm."""
    from opentransformer_amd import ops
    try:
        cfg, model, lm, lm_cfg, x, m = _setup('fp32', lm_kind)
        beam, max_len, lw = 5, 32, 0.3                     # max_len > T' (29): every hypothesis ends in EOS, CTC sees to that
        for lam in (0.3, 0.7):
            want_h, want_s, (dec, clp, cln, lm_fn) = _restated(cfg, model, lm, lm_cfg, x, m, beam, max_len, lam, lw, 7, 3)
            assert len(want_h[2][0]) <= int(cln[2])
            for cache in (False, True):
                nb, sc = _rec(model, lm, beam_width=beam, nbest=3, max_len=max_len, lm_weight=lw, ctc_weight=lam, joint_ctc=True,
                              apply_cache=cache).recognize(x, m)
                assert _tok(nb) == want_h, (lam, cache)
                np.testing.assert_allclose(sc.numpy(), want_s.numpy(), rtol=1e-5, atol=1e-4)
                if cache:
                    got_s = sc
            # telescoping, computed independently (teacher-forced oracle decoder, torch's CTC loss, the oracle LM)
            with torch.no_grad():
                mem, mm, _, _ = _rec(model, None).encode(x, m)
            mem, mm = mem.float().cpu(), mm.cpu()
            checked = 0
            for b in range(4):
                y = want_h[b][0]
                if len(y) >= max_len:
                    continue
                tin = torch.tensor([[EOS] + y])
                tout = y + [EOS]
                att = F.log_softmax(orc.transformer_decoder(dec, tin, mem[b:b + 1], mm[b:b + 1], cfg['decoder']), -1)[0]
                s_att = float(sum(att[i, t] for i, t in enumerate(tout)))
                if y:
                    nll = F.ctc_loss(clp[b:b + 1].transpose(0, 1).double(), torch.tensor([y]), cln[b:b + 1], torch.tensor([len(y)]),
                                     blank=BLANK, reduction='none')
                    s_ctc = -float(nll[0])
                else:
                    s_ctc = float(clp[b, :int(cln[b]), BLANK].double().sum())
                s_lm = 0.0
                if lm_fn is not None:
                    s_lm = float(sum(lm_fn(tin[:, :i + 1])[0, t] for i, t in enumerate(tout)))
                tele = (1 - lam) * s_att + lam * s_ctc + lw * s_lm
                assert abs(tele - float(got_s[b, 0])) < 1e-3, (b, tele, float(got_s[b, 0]))
                checked += 1
            assert checked >= 3
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_lambda_zero_is_the_plain_search(mode):
    """joint_ctc=True, ctc_weight=0 returns exactly the hypotheses and scores of joint_ctc=False, in both loops"""
    from opentransformer_amd import ops
    try:
        _, model, lm, _, x, m = _setup(mode, 'transformer')
        for cache in (False, True):
            kw = dict(beam_width=5, nbest=5, max_len=10, lm_weight=0.3, penalty=0.6, apply_cache=cache)
            h0, s0 = _rec(model, lm, ctc_weight=0.0, **kw).recognize(x, m)
            h1, s1 = _rec(model, lm, ctc_weight=0.0, joint_ctc=True, **kw).recognize(x, m)
            assert h0 == h1, cache
            assert torch.equal(s0, s1), cache
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('mode', ['bf16', 'fp16'])
def test_joint_cached_matches_reforward_16bit(mode):
    from opentransformer_amd import ops
    try:
        _, model, lm, _, x, m = _setup(mode, 'transformer')
        kw = dict(beam_width=5, nbest=2, max_len=10, lm_weight=0.3, ctc_weight=0.3, joint_ctc=True)
        h0, s0 = _rec(model, lm, apply_cache=False, **kw).recognize(x, m)
        h1, s1 = _rec(model, lm, apply_cache=True, **kw).recognize(x, m)
        clear = (s0[:, 0] - s0[:, 1]) > 0.1
        assert clear.sum() >= 2
        for b in range(4):
            if clear[b]:
                assert h0[b][0] == h1[b][0], b
                assert abs(float(s0[b, 0]) - float(s1[b, 0])) < 5e-2
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('case', ['transformer', 'rnn', 'lookahead'])
def test_joint_graph_replay_and_state_reuse(case):
    """one recognizer (one CachedBeamState, replayed graphs) over two different batches = fresh recognizers, and eager = graph"""
    from opentransformer_amd import ops
    try:
        cfg = syn.c1_lookahead(2) if case == 'lookahead' else None
        lm_kind = None if case == 'lookahead' else case
        _, model, lm, _, x, m = _setup('fp32', lm_kind, cfg=cfg)
        _, _, _, _, x2, m2 = _setup('fp32', None, cfg=cfg, seed=12)
        kw = dict(beam_width=4, nbest=2, max_len=8, lm_weight=0.3, ctc_weight=0.5, joint_ctc=True, apply_cache=True)
        shared = _rec(model, lm, **kw)
        got = [shared.recognize(x, m), shared.recognize(x2, m2), shared.recognize(x, m)]
        for (xx, mm), g in zip(((x, m), (x2, m2), (x, m)), got):
            fresh = _rec(model, lm, **kw)
            fresh.use_hipgraph = False
            want = fresh.recognize(xx, mm)
            assert g[0] == want[0]
            np.testing.assert_allclose(g[1].numpy(), want[1].numpy(), rtol=1e-5, atol=1e-5)
            ref_h = _rec(model, lm, **dict(kw, apply_cache=False)).recognize(xx, mm)
            assert ref_h[0] == want[0]
    finally:
        ops.set_compute_dtype('bf16')
