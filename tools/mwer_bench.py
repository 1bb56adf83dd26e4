"""MWER training benchmark (ops.mwer_loss / otr_mwer_loss, MWERTraining) at B 32, N 4, max_len 32 (the fused decoder stack's limit),
V 4234 (row stride 4240), C2 model.  Two parts, one JSON line:
 (a) otr_mwer_loss forward + gradient on preallocated buffers, against the same loss composed from torch ops (log_softmax over
     [B*N*L, V], gather, masked sum, softmax, mean; autograd for the gradient) on the same logits in the same run, and against the time
     of its own traffic -- two reads of the live rows plus one write of the whole gradient -- at the 8 TB/s HBM figure of DESIGN.md.
     The composed route's loss and gradient are checked against the kernel's.
 (b) one MWER train step (forward + backward, eager, no optimizer) split into search / forward (scoring pass + loss) / the loss launches
     alone / backward, against the cross-entropy step of the same model on the same batch in the same run.  The search is timed for the
     re-forward loop, for the cached loop with its graphs alive, and for the cached loop after a weight update (its captured graphs are
     keyed by the weights' version: it rebuilds them), which is what a training step sees.  The step itself runs on fixed hypotheses of
     the references' lengths (an untrained model's own search runs to max_len and leaves nothing to score).
Warm-up, then timed repeats with device events; medians.

    python tools/mwer_bench.py [--iters 20] [--search-iters 3] [--frames 1000] [--mode fp16] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opentransformer_amd as ota                        # noqa: E402
from opentransformer_amd import _lib as L, ops, synthetic as syn          # noqa: E402

HBM_BYTES_PER_S = 8e12
B, N, MAX_LEN, V, LD = 32, 4, 32, 4234, 4240


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def composed(logits, ys_out, n_rows, errors):
    nh, ml, _ = logits.shape
    lp = torch.log_softmax(logits, dim=-1)
    tok = lp.gather(-1, ys_out.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    rows = torch.arange(ml, device=logits.device).unsqueeze(0) < n_rows.unsqueeze(1)
    s = torch.where(rows, tok, torch.zeros_like(tok)).sum(-1).view(errors.shape)
    live = (n_rows.view(errors.shape) > 0) & (errors >= 0)
    post = torch.softmax(s.masked_fill(~live, float('-inf')), dim=-1)
    return (post * errors.clamp(min=0).float()).sum(-1).mean()


def kernel_part(iters):
    rng = np.random.default_rng(0)
    dev = 'cuda'
    nh = B * N
    full = torch.from_numpy(rng.normal(size=(nh * MAX_LEN, LD)).astype(np.float32)).to(dev)
    lens = rng.integers(10, MAX_LEN - 1, size=nh)         # tokens per hypothesis; rows = tokens + 1
    n_rows = torch.from_numpy((lens + 1).astype(np.int32)).to(dev)
    ys = -np.ones((nh, MAX_LEN), np.int64)
    for h in range(nh):
        ys[h, :lens[h]] = rng.integers(2, V, size=lens[h])
        ys[h, lens[h]] = 1
    ys_out = torch.from_numpy(ys).to(dev)
    errors = torch.from_numpy(rng.integers(0, 8, size=(B, N)).astype(np.int32)).to(dev)
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)    # noqa: E731
    loss, seq, post, utt, dl = f32(1), f32(nh), f32(B, N), f32(B), f32(nh * MAX_LEN, LD)
    nws = lib.otr_mwer_workspace_floats(B, N, MAX_LEN)
    ws = f32(nws)

    def launch(grad=True):
        L.check(lib.otr_mwer_loss(p(full), LD, p(ys_out), MAX_LEN, p(n_rows), p(errors), B, N, MAX_LEN, V, None, p(loss), p(seq), p(post),
                                  p(utt), p(dl) if grad else None, LD, p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                'otr_mwer_loss')
    view = full[:, :V].view(nh, MAX_LEN, V)
    leaf = full.clone().requires_grad_(True)

    def torch_route():
        leaf.grad = None
        composed(leaf[:, :V].view(nh, MAX_LEN, V), ys_out, n_rows, errors).backward()
    t_kernel = timed(launch, iters)
    t_fwd = timed(lambda: launch(False), iters)
    t_torch = timed(torch_route, iters)
    t_torch_fwd = timed(lambda: composed(view, ys_out, n_rows, errors), iters)
    launch()
    torch_route()
    want = composed(view, ys_out, n_rows, errors)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(want)) < 1e-3, (float(loss), float(want))
    gerr = float((dl - leaf.grad).abs().max() / leaf.grad.abs().max())
    assert gerr < 1e-3, gerr
    live_rows = int(n_rows.sum())
    traffic = (2 * live_rows * V + nh * MAX_LEN * LD) * 4
    floor_ms = traffic / HBM_BYTES_PER_S * 1e3
    return {'kernel_fwd_grad_ms': round(t_kernel, 4), 'kernel_fwd_only_ms': round(t_fwd, 4), 'torch_fwd_grad_ms': round(t_torch, 4),
            'torch_fwd_only_ms': round(t_torch_fwd, 4), 'torch_over_kernel': round(t_torch / t_kernel, 2),
            'kernel_not_slower_than_torch': bool(t_kernel <= t_torch), 'live_rows': live_rows, 'rows': nh * MAX_LEN,
            'traffic_mb': round(traffic / 1e6, 1), 'traffic_floor_ms_at_8TBps': round(floor_ms, 4),
            'kernel_over_floor': round(t_kernel / floor_ms, 2), 'grad_rel_diff_vs_torch': gerr}


def step_part(a):
    dev = 'cuda'
    ops.set_compute_dtype(a.mode)
    model = ota.SpeechToText(syn.c2_model(0.1))
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(dev).train()
    inputs, targets = syn.synthetic_batch(B, a.frames, 80, V, 15, seed=0)
    inputs = {k: v.to(dev) for k, v in inputs.items()}
    targets = {k: v.to(dev) for k, v in targets.items()}
    wrap = ota.MWERTraining(model, nbest=N, max_len=MAX_LEN)
    # fixed hypotheses: the reference and three copies with one, two and three substitutions
    truth = targets['targets']
    k = int(targets['targets_length'].max()) - 1
    tokens = truth[:, 1:1 + k].unsqueeze(1).repeat(1, N, 1).contiguous()
    for n in range(1, N):
        tokens[:, n, :n] = 2 + (tokens[:, n, :n] + 7) % (V - 2)
    lengths = (targets['targets_length'] - 1).to(torch.int32).unsqueeze(1).repeat(1, N).contiguous()
    hyps = (tokens, lengths)
    out = {}

    def bump():
        with torch.no_grad():
            for p_ in model.parameters():
                p_.add_(0)
    search = lambda: wrap.search(inputs['inputs'], inputs['mask'])        # noqa: E731
    out['search_reforward_ms'] = round(timed(search, a.search_iters, warmup=1), 3)
    wrap.recognizer.apply_cache = True
    out['search_cached_ms'] = round(timed(search, a.search_iters, warmup=1), 3)
    out['search_cached_after_weight_update_ms'] = round(timed(lambda: (bump(), search()), a.search_iters, warmup=1), 3)
    wrap.recognizer.apply_cache = False
    wrap.recognizer._cached_states.clear()
    tok, ln = search()
    out['search_mean_hyp_tokens'] = round(float(ln.float().mean()), 1)

    state = {}

    def clear():
        for p_ in model.parameters():
            p_.grad = None

    def mwer_fwd():
        clear()
        state['loss'] = wrap(inputs, targets, hyps=hyps)[0]

    def ce_fwd():
        clear()
        state['loss'] = model(inputs, targets)[0]

    def split(fwd):
        def both():
            fwd()
            ops.backward(state['loss'])
        t_fwd = timed(fwd, a.iters)
        t_both = timed(both, a.iters)
        return t_fwd, t_both - t_fwd, t_both
    f, b, t = split(mwer_fwd)
    rec = []
    ops.set_kernel_timer(rec)
    try:
        for _ in range(5):
            mwer_fwd()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    t_loss = float(np.median([e0.elapsed_time(e1) for name, _, e0, e1, _ in rec if name.startswith('mwer_loss')]))
    out.update(mwer_forward_ms=round(f, 3), mwer_loss_launches_ms=round(t_loss, 4), mwer_scoring_pass_ms=round(f - t_loss, 3),
               mwer_backward_ms=round(b, 3), mwer_step_ms=round(t, 3))
    f, b, t = split(ce_fwd)
    out.update(ce_forward_ms=round(f, 3), ce_backward_ms=round(b, 3), ce_step_ms=round(t, 3))
    out['mwer_step_over_ce_step'] = round(out['mwer_step_ms'] / out['ce_step_ms'], 2)
    best = min(out['search_reforward_ms'], out['search_cached_after_weight_update_ms'])
    out['mwer_step_with_search_over_ce_step'] = round((out['mwer_step_ms'] + best) / out['ce_step_ms'], 2)
    out['faster_training_search'] = 'reforward' if out['search_reforward_ms'] <= out['search_cached_after_weight_update_ms'] else 'cached'
    ops.set_compute_dtype('bf16')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--search-iters', type=int, default=3)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--no-step', action='store_true', help='part (a) only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mwer_bench needs a GPU')
    res = {'shape': {'B': B, 'N': N, 'max_len': MAX_LEN, 'V': V, 'ld': LD}, 'iters': a.iters, 'kernel': kernel_part(a.iters)}
    if not a.no_step:
        res['step'] = dict(step_part(a), mode=a.mode, frames=a.frames, model='c2')
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
