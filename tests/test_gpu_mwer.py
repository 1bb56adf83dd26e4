"""GPU (-m gpu): minimum word error rate training.  otr_mwer_loss (csrc/mwer.hip) against the numpy float64 restatement
(tests/mwer_ref.py) on the aligned and the scalar row routes, ops.mwer_loss through autograd, and MWERTraining against the same model
with the loss composed from torch ops in float64 on the same logits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opentransformer_amd import synthetic as syn
from tests import helpers as H
from tests import mwer_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, MAX_LEN = 4, 9


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(V, pad, N, extra=False):
    """the recipe of the issue (tests/mwer_ref.case) and what the restatement makes of it, computed once per shape"""
    rng = np.random.default_rng(V * 100 + pad * 7 + N)
    x, ys_out, n_rows, errors = ref.case(rng, B, N, MAX_LEN, V)
    if extra:                                               # utterance 2 without a live slot, one invalid pair in utterance 3
        n_rows[2 * N:3 * N] = 0
        errors[3, 0] = -1
    lg = rng.normal(size=(B * N * MAX_LEN, V + pad)).astype(np.float32)      # the pad columns hold numbers too: they must not matter
    lg[:, :V] = x.reshape(-1, V).astype(np.float32)
    x32 = lg[:, :V].reshape(B * N, MAX_LEN, V)
    want = ref.forward(x32, ys_out, n_rows, errors, V)
    want['grad'] = ref.grad(x32, ys_out, n_rows, errors, V)
    return lg, ys_out, n_rows, errors, want


def _run(lg_d, V, ys, nr, er, N, grad=True, gscale=None, ldd=None):
    """otr_mwer_loss through the library's own entry: logits as a view with row stride ld = V + pad, the gradient into a buffer
    pre-filled with NaN; returns the outputs as numpy arrays (dlogits at its full width)"""
    from opentransformer_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    nh = B * N
    ld = lg_d.stride(0)
    ldd = ld if ldd is None else ldd
    out = {k: torch.full(sh, float('nan'), device=DEV) for k, sh in (('loss', (1,)), ('seq_logp', (nh,)), ('post', (B, N)), ('utt_err', (B,)))}
    dl = torch.full((nh * MAX_LEN, ldd), float('nan'), device=DEV) if grad else None
    nws = lib.otr_mwer_workspace_floats(B, N, MAX_LEN)
    assert nws == nh * MAX_LEN + nh
    ws = torch.empty(nws, device=DEV)
    rc = lib.otr_mwer_loss(p(lg_d), ld, p(ys), ys.stride(0), p(nr), p(er), B, N, MAX_LEN, V, p(gscale), p(out['loss']), p(out['seq_logp']),
                           p(out['post']), p(out['utt_err']), p(dl), ldd, p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.otr_last_error_string()
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['dlogits'] = dl.cpu().numpy() if grad else None
    return res


def _check(got, want, V, N, n_rows, errors, scale=1.0):
    s_want = want['seq_logp'].reshape(-1)
    live = want['live'].reshape(-1)
    eps = 1e-4 + 1e-6 * np.abs(s_want[live]).max() if live.any() else 1e-4       # f32 sums of up to max_len rows (tests/test_gpu_rescore.py)
    w_max = max(1, int(errors.max()))
    print('mwer V=%d N=%d: max |s err| %.3g (eps %.3g), |post err| %.3g, |utt_err err| %.3g, |loss err| %.3g (bound %.3g)' % (
        V, N, np.abs(got['seq_logp'][live] - s_want[live]).max() if live.any() else 0, eps, np.abs(got['post'] - want['post']).max(),
        np.abs(got['utt_err'] - want['utt_err']).max(), abs(got['loss'][0] - want['loss']), 4 * eps * w_max))
    assert np.array_equal(got['seq_logp'] == -np.inf, ~live)
    assert np.all(np.abs(got['seq_logp'][live] - s_want[live]) <= 1e-4 + 1e-6 * np.abs(s_want[live]))
    assert np.all(np.abs(got['post'] - want['post']) <= 4 * eps * w_max) and np.all(got['post'][~want['live']] == 0)
    assert np.all(np.abs(got['utt_err'] - want['utt_err']) <= 4 * eps * w_max)
    assert abs(got['loss'][0] - want['loss']) <= 4 * eps * w_max
    d = got['dlogits']
    if d is None:
        return
    d3 = d.reshape(B * N, MAX_LEN, -1)
    g_want = scale * want['grad']
    err = np.abs(d3[:, :, :V] - g_want)
    bound = 1e-6 * scale + 1e-3 * np.abs(g_want)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print('  dlogits: max |err| %.3g, worst margin at %s: err %.3g bound %.3g' % (err.max(), worst, err[worst], bound[worst]))
    assert np.all(err <= bound)
    assert np.all(d3[:, :, V:] == 0)                        # the pad columns (a NaN would fail the comparison)
    for h in range(B * N):
        rows = n_rows[h] if live[h] else 0
        assert np.all(d3[h, rows:] == 0), h                 # rows at or past n_rows, dead slots: exactly zero


@pytest.mark.parametrize('V,pad', [(100, 0), (100, 4), (4233, 0), (4233, 7), (4234, 6), (8192, 0), (8192, 3)])
@pytest.mark.parametrize('N', [1, 2, 5, 32])
def test_kernel_matches_restatement(V, pad, N):
    lg, ys_out, n_rows, errors, want = _case(V, pad, N)
    live = want['live']
    if N >= 2:      # the test cannot pass on vanishing gradients: a third of the live slots carry a weight above 1e-3
        assert (np.abs(want['c'][live]) > 1e-3).sum() * 3 >= live.sum(), ((np.abs(want['c'][live]) > 1e-3).sum(), live.sum())
    if N >= 5:
        assert (~live).sum() == 1 and n_rows[1 * N + 2] == MAX_LEN - 1
    lg_d = _dev(lg)[:, :V] if pad else _dev(lg)             # ld > V: a view with a longer row stride
    ys, nr, er = _dev(ys_out), _dev(n_rows), _dev(errors)
    got = _run(lg_d, V, ys, nr, er, N)
    _check(got, want, V, N, n_rows, errors)
    again = _run(lg_d, V, ys, nr, er, N)
    for k in got:
        assert np.array_equal(got[k], again[k]), k          # the same bits on every run
    fwd = _run(lg_d, V, ys, nr, er, N, grad=False)
    for k in ('loss', 'seq_logp', 'post', 'utt_err'):
        assert np.array_equal(got[k], fwd[k]), k            # dlogits = NULL: the same forward outputs
    scaled = _run(lg_d, V, ys, nr, er, N, gscale=torch.tensor([1024.0], device=DEV))
    assert np.array_equal(scaled['dlogits'], 1024.0 * got['dlogits'])
    assert np.array_equal(scaled['loss'], got['loss'])
    narrow = _run(lg_d, V, ys, nr, er, N, ldd=V)            # the gradient at its own width: another alignment of the stores
    assert np.array_equal(narrow['dlogits'], got['dlogits'][:, :V])
    x = lg[:, :V].reshape(B * N, MAX_LEN, V).astype(np.float64)
    g = got['dlogits'].reshape(B * N, MAX_LEN, -1)[:, :, :V].astype(np.float64)
    if N == 1:
        assert not g.any() and got['loss'][0] == errors.mean()          # one hypothesis: its errors, no gradient
    else:
        after = ref.forward(x - 0.1 * g, ys_out, n_rows, errors, V)['loss']
        assert after < want['loss'], (after, want['loss'])  # descent on the device's gradient


@pytest.mark.parametrize('V,pad', [(100, 4), (4233, 0)])
def test_dead_utterance_and_invalid_pair(V, pad):
    N = 5
    lg, ys_out, n_rows, errors, want = _case(V, pad, N, True)
    assert want['b_live'] == 3 and not want['live'][2].any() and not want['live'][3, 0]
    lg_d = _dev(lg)[:, :V] if pad else _dev(lg)
    got = _run(lg_d, V, _dev(ys_out), _dev(n_rows), _dev(errors), N)
    _check(got, want, V, N, n_rows, errors)
    assert got['utt_err'][2] == 0
    # a target outside the vocabulary kills its slot; no live slot anywhere gives loss 0 and an all-zero gradient
    y2 = ys_out.copy()
    y2[0, 0] = V
    x32 = lg[:, :V].reshape(B * N, MAX_LEN, V)
    w2 = ref.forward(x32, y2, n_rows, errors, V)
    w2['grad'] = ref.grad(x32, y2, n_rows, errors, V)
    assert not w2['live'][0, 0]
    _check(_run(lg_d, V, _dev(y2), _dev(n_rows), _dev(errors), N), w2, V, N, n_rows, errors)
    none = _run(lg_d, V, _dev(ys_out), _dev(np.zeros_like(n_rows)), _dev(errors), N)
    assert none['loss'][0] == 0 and not none['dlogits'].any() and not none['post'].any() and np.all(none['seq_logp'] == -np.inf)


# ---------------------------------------------------------------- ops.mwer_loss through autograd
def _composed(logits, ys_out, n_rows, errors, dtype):
    """the same loss from torch ops: log_softmax over [B*N*L, V], gather, masked sum, softmax over the live slots"""
    nh, ml, _ = logits.shape
    Bn, N = errors.shape
    lp = torch.log_softmax(logits.to(dtype), dim=-1)
    tok = lp.gather(-1, ys_out.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    rows = torch.arange(ml, device=logits.device).unsqueeze(0) < n_rows.unsqueeze(1)
    s = torch.where(rows, tok, torch.zeros_like(tok)).sum(-1).view(Bn, N)
    live = (n_rows.view(Bn, N) > 0) & (errors >= 0)
    post = torch.softmax(s.masked_fill(~live, float('-inf')), dim=-1)
    exp_err = (post * errors.clamp(min=0).to(dtype)).sum(-1)
    return exp_err.mean(), s, post


def test_op_gradient_through_a_row_padded_view():
    """ops.mwer_loss on the [R, V] head of a [R, V8] product: the gradient of the padded leaf is the kernel's, zero in the tail, and
    a seed other than ops.backward's unit scalar multiplies it"""
    from opentransformer_amd import ops
    V, pad, N = 4234, 6, 5
    lg, ys_out, n_rows, errors, want = _case(V, pad, N)
    ys, nr, er = _dev(ys_out), _dev(n_rows), _dev(errors)
    direct = _run(_dev(lg)[:, :V], V, ys, nr, er, N)
    full = _dev(lg).requires_grad_(True)
    loss, stats = ops.mwer_loss(full[:, :V].view(B * N, MAX_LEN, V), ys, nr, er)
    assert not stats['post'].requires_grad and stats['seq_logp'].shape == (B, N)
    ops.backward(loss)
    torch.cuda.synchronize()
    assert loss.item() == float(direct['loss'][0])
    assert np.array_equal(full.grad.cpu().numpy(), direct['dlogits'])
    assert np.array_equal(stats['post'].cpu().numpy(), direct['post'])
    full2 = _dev(lg).requires_grad_(True)
    loss2, _ = ops.mwer_loss(full2[:, :V].view(B * N, MAX_LEN, V), ys, nr, er)
    (loss2 * 3.0).backward()
    np.testing.assert_allclose(full2.grad.cpu().numpy(), 3.0 * direct['dlogits'], rtol=1e-6, atol=0)
    with torch.no_grad():                                   # no gradient wanted: forward only
        loss3, _ = ops.mwer_loss(full[:, :V].view(B * N, MAX_LEN, V), ys, nr, er)
    assert loss3.item() == loss.item() and not loss3.requires_grad


# ---------------------------------------------------------------- model level
def _model_case(mode):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    ops.set_compute_dtype(mode)
    cfg = syn.c1_model(0.0) if mode == 'fp32' else syn.c2_model(0.0, n_enc=1, n_dec=2)
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).train()
    V = model.decoder.output_layer.weight.shape[0]
    inputs, targets = syn.synthetic_batch(4, 96, 80, V, 6, seed=5, lengths=[96, 80, 96, 64], tgt_lengths=[6, 4, 5, 6])
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    max_len, L = 8, 9
    truth, n = targets['targets'], targets['targets_length'] - 1
    tokens = torch.full((4, 3, L), 1, dtype=torch.int64, device=DEV)
    lengths = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(7)
    for b in range(4):
        k = int(n[b])
        tokens[b, 0, :k] = truth[b, 1:1 + k]                # the reference itself
        bad = truth[b, 1:1 + k].clone()
        for j in (1, k - 1):                                # a corrupted copy of the same length: two substitutions
            bad[j] = 2 + (int(bad[j]) + 5) % (V - 2)
        tokens[b, 1, :k] = bad
        tokens[b, 2, :max_len] = torch.randint(2, V, (max_len,), generator=g).to(DEV)     # longer than max_len - 1: takes no part
        lengths[b] = torch.tensor([k, k, max_len], dtype=torch.int32)
    return model, inputs, targets, (tokens, lengths), max_len, V


def _composed_step(model, inputs, targets, hyps, max_len, V, ce_weight, dtype):
    """MWERTraining.forward with the loss (and only the loss) composed from torch ops in `dtype` on the model's own logits"""
    from opentransformer_amd import ops
    tokens, lengths = hyps
    Bn, N, _ = tokens.shape
    truth = targets['targets']
    errors = ops.edit_distance(truth[:, 1:], targets['targets_length'] - 1, tokens, lengths)[0]
    ys_in, ys_out, n_rows = ops.rescore_pack(tokens, lengths, torch.zeros((Bn, N), device=DEV), max_len, V, 1, 1)
    x, mask = model.frontend(inputs['inputs'], inputs['mask'])
    memory, memory_mask, _ = model.encoder(x, mask)
    logits = ops.linear(model.decoder.hidden(ys_in, memory, memory_mask, share=N), model.decoder.output_layer.weight,
                        model.decoder.output_layer.bias)
    mwer, s, _ = _composed(logits, ys_out, n_rows, errors, dtype)
    total = mwer.float()
    if ce_weight > 0:
        ce_logits, _ = model.decoder(truth[:, :-1], memory, memory_mask)
        total = total + ce_weight * model.crit(ce_logits, truth[:, 1:])
    return total, mwer, s, errors


def _grads(model, loss):
    from opentransformer_amd import ops
    for p in model.parameters():
        p.grad = None
    ops.backward(loss)
    torch.cuda.synchronize()
    named = [(n, p.grad.detach().clone()) for n, p in model.named_parameters() if p.grad is not None]
    return [n for n, _ in named], [g for _, g in named]


@pytest.mark.parametrize('ce_weight', [0.01, 0.0])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_training_step_matches_the_composed_loss(mode, ce_weight):
    """MWERTraining.forward + ops.backward against the same model with the loss composed from torch ops in float64 on the same
    logits.  Loss: the kernel bound 4 eps max(1, W_max).  Parameter gradients (tests.helpers.key_aware_grad_errors): max(1e-4, 4 d0),
    1e-4 the fp32-mode training bar and d0 the distance between the composed route with float32 and with float64
    loss math -- what fp32 rounding of dlogits alone does to the same backward pass; the factor 4 covers the other summation order."""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets, hyps, max_len, V = _model_case(mode)
        wrap = ota.MWERTraining(model, nbest=3, max_len=max_len, ce_weight=ce_weight)
        assert model.training and wrap.model is model
        loss, aux = wrap(inputs, targets, hyps=hyps)
        names, got = _grads(model, loss)
        total64, mwer64, s64, errors = _composed_step(model, inputs, targets, hyps, max_len, V, ce_weight, torch.float64)
        names64, want = _grads(model, total64)
        total32, _, _, _ = _composed_step(model, inputs, targets, hyps, max_len, V, ce_weight, torch.float32)
        _, base = _grads(model, total32)
        assert names == names64 and len(names) > 10
        assert torch.equal(aux['errors_1best'], errors[:, 0]) and int(errors[:, 0].abs().sum()) == 0         # slot 0 is the reference
        assert torch.equal(aux['errors_oracle'], errors[:, :2].min(dim=1).values) and bool((errors[:, 1] == 2).all())
        assert bool((aux['post'][:, 2] == 0).all()) and bool((aux['post'][:, :2] > 0).all())                  # the long slot takes no part
        print('mwer model %s ce=%g: posteriors %s' % (mode, ce_weight, aux['post'][:, :2].tolist()))
        # two hypotheses of one length on an untrained model: the posterior is split, so the gradient weights P (W - E) / B are not vanishing
        assert int((aux['post'][:, :2].min(dim=1).values > 1e-2).sum()) >= 2
        eps = 1e-4 + 1e-6 * float(s64[:, :2].abs().max())
        w_max = max(1, int(errors.max()))
        print('mwer model %s ce=%g: MWER %.6f composed %.6f, total %.6f composed %.6f' % (
            mode, ce_weight, float(aux["MWER"]), mwer64.item(), loss.item(), total64.item()))
        assert abs(float(aux["MWER"]) - mwer64.item()) <= 4 * eps * w_max
        assert abs(loss.item() - total64.item()) <= 4 * eps * w_max + 1e-6 * abs(total64.item())
        d_model = model.decoder.d_model
        errs, key_errs = H.key_aware_grad_errors(names, got, want, d_model)
        d0, _ = H.key_aware_grad_errors(names, base, want, d_model)
        worst = max(errs, key=lambda k: errs[k] / max(1e-4, 4 * d0[k]))
        print('  grads: worst %s err %.3g bound %.3g; max err %.3g, max d0 %.3g, max key residue %.3g' % (
            worst, errs[worst], max(1e-4, 4 * d0[worst]), max(errs.values()), max(d0.values()), max(key_errs.values(), default=0.0)))
        assert len(errs) > 10
        for k, e in errs.items():
            assert e <= max(1e-4, 4 * d0[k]), (k, e, d0[k])
    finally:
        ops.set_compute_dtype('bf16')


def _trained_c1(golden, dropout):
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    g = golden('c1_decode.npz')
    ops.set_compute_dtype('fp32')
    model = ota.SpeechToText(syn.c1_model(dropout, ctc_weight=0.3))
    model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w:')}, strict=True)
    inputs = {'inputs': torch.from_numpy(g['inputs']).to(DEV), 'mask': torch.from_numpy(g['mask']).to(DEV)}
    rng = np.random.default_rng(3)
    tg = np.zeros((4, 8), np.int64)
    lens = [5, 6, 3, 4]
    for b, k in enumerate(lens):
        tg[b, 0], tg[b, 1:1 + k], tg[b, 1 + k] = 1, rng.integers(2, 100, size=k), 1
    targets = {'targets': torch.from_numpy(tg).to(DEV), 'targets_length': torch.tensor([k + 1 for k in lens], dtype=torch.int32, device=DEV)}
    return model.to(DEV), inputs, targets


def test_search_inside_the_step(golden):
    """hyps=None on the trained C1 model with dropout 0.1 in train(): the n-best is the recognizer's own, the modes are restored (also
    when the search raises), everything is finite, and a second step after a weight update still works"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    try:
        model, inputs, targets = _trained_c1(golden, 0.1)
        model.train()
        wrap = ota.MWERTraining(model, nbest=3, beam_width=4, max_len=12)
        assert model.training and all(m.training for m in model.modules())       # the recognizer's eval() was undone
        assert not wrap.recognizer.apply_cache
        loss, aux = wrap(inputs, targets)
        assert model.training and all(m.training for m in model.modules())
        ops.backward(loss)
        torch.cuda.synchronize()
        model.eval()
        with torch.no_grad():
            tokens, lengths, _ = wrap.recognizer.recognize_tokens(inputs['inputs'], inputs['mask'])
        dist = ops.edit_distance(targets['targets'][:, 1:], targets['targets_length'] - 1, tokens, lengths)[0]
        assert tokens.shape[:2] == (4, 3) and int(lengths.max()) > 0
        assert torch.equal(aux['errors_1best'], dist[:, 0]) and torch.equal(aux['errors_oracle'], dist.min(dim=1).values)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(aux['MWER'])) and bool(torch.isfinite(aux['CE']))
        assert float(aux['post'].sum()) > 0
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
        assert sum(float(g.abs().sum()) for g in grads) > 0
        wrap(inputs, targets)
        assert not model.training and not any(m.training for m in model.modules())    # a model in eval() stays in eval()
        model.train()
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0)                                   # a fake optimizer step: every weight's version moves on
        loss2, _ = wrap(inputs, targets)
        ops.backward(loss2)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss2)) and model.training

        def boom(*a, **k):
            raise RuntimeError('search failed')
        wrap.recognizer.recognize_tokens = boom
        with pytest.raises(RuntimeError, match='search failed'):
            wrap(inputs, targets)
        assert model.training and all(m.training for m in model.modules())
    finally:
        ops.set_compute_dtype('bf16')
