"""The transducer, benchmark (ops.rnnt_loss / otr_rnnt_loss, ops.rnnt_joint, TransducerModel, TransducerRecognizer).  One JSON line:
 (0) before anything is timed, at the loss bench shape (B 32, T' 250, U + 1 21, V 4233): nll and the gradient slab of utterances 0 and
     31 (the one whose byte offsets pass 2^32) against the float64 restatement of tests/rnnt_ref.py on the CPU;
 (a) the loss on those logits: ops.rnnt_loss forward + gradient and forward only, and the entry's own launches split into its passes by
     differences of timings -- the lattice and mean launches as the same entry on two-column logits, the row pass as what the
     forward-only call takes beyond that, the gradient pass as what the call with a gradient takes beyond the forward-only call --
     the row and gradient passes each against their minimum HBM traffic (the row pass reads the live rows once, the gradient pass
     reads them again and writes every row) at the 8 TB/s figure of DESIGN.md; and the same loss composed from torch ops in the same run (log_softmax, gather, one logaddexp per anti-diagonal,
     autograd), at the same shape if memory allows, otherwise at the largest batch that does -- the line says which;
 (b) the joint at J 512: ops.rnnt_joint forward and forward + backward against their traffic;
 (c) the C2 encoder in fp16 with joint_size 512, B 32, 1000 frames, eager: the whole train step (forward + backward, no optimizer) and
     a greedy decode of the batch.
Warm-up, then timed repeats with device events; medians.

    python tools/rnnt_bench.py [--iters 10] [--frames 1000] [--mode fp16] [--no-step] [--out f.json]
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
from tests import rnnt_ref as rr                         # noqa: E402

HBM_BYTES_PER_S = 8e12
B, T, U1, V, J = 32, 250, 21, 4233, 512
DEV = 'cuda'
NEG = -1e30
CHECK_K = 4.0                 # half of tests/test_gpu_rnnt.py's K: the bench shape meets it (profiles/rnnt_bench.json)


def timed(fn, iters, warmup=2):
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


def torch_rnnt(x, el, labels, tl):
    """the loss from torch ops on the device, batched: one logaddexp per anti-diagonal (tests/rnnt_ref.py's sweep over [B, U1])"""
    Bx, Tx, Ux, _ = x.shape
    lp = torch.log_softmax(x, dim=-1)
    lpb = lp[..., 0]
    lpl = lp[:, :, :-1].gather(3, labels[:, None, :Ux - 1, None].expand(Bx, Tx, Ux - 1, 1))[..., 0]
    u = torch.arange(Ux, device=x.device)
    el, tl = el.long(), tl.long()
    neg = x.new_full((), NEG)
    prev = torch.where(u == 0, x.new_zeros(()), neg).expand(Bx, Ux)
    last = el - 1 + tl
    final = torch.where(last == 0, x.new_zeros(Bx), x.new_full((Bx,), NEG))
    pad = x.new_full((Bx, 1), NEG)
    zero = x.new_zeros((Bx, 1))
    for d in range(1, Tx + Ux - 1):
        t = d - u
        tc = t.clamp(0, Tx - 1)
        live = (t >= 0)[None, :] & (t[None, :] < el[:, None]) & (u[None, :] <= tl[:, None])
        up = prev + lpb[:, (tc - 1).clamp(min=0), u]
        left = torch.cat((pad, prev[:, :-1]), 1) + torch.cat((zero, lpl[:, tc[1:], u[1:] - 1]), 1)
        cur = torch.logaddexp(torch.where(live & (t >= 1)[None, :], up, neg), torch.where(live & (u >= 1)[None, :], left, neg))
        prev = torch.where(live, cur, neg)
        final = torch.where(last == d, prev.gather(1, tl[:, None])[:, 0], final)
    ar = torch.arange(Bx, device=x.device)
    nll = -(final + lpb[ar, el - 1, tl])
    return nll.mean(), nll


def make_batch(seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = torch.randn((B, T, U1, V), generator=g, device=DEV, dtype=torch.float32)
    rng = np.random.default_rng(seed)
    el = torch.from_numpy(rng.integers(T - 40, T + 1, size=B).astype(np.int32))
    tl = torch.from_numpy(rng.integers(U1 - 6, U1, size=B).astype(np.int32))
    el[0], tl[0], el[B - 1], tl[B - 1] = T, U1 - 1, T, U1 - 1          # the two checked utterances use the whole lattice
    labels = torch.from_numpy(rng.integers(1, V, size=(B, U1 - 1)).astype(np.int64))
    return logits, el.to(DEV), labels.to(DEV), tl.to(DEV)


def check_part(logits, el, labels, tl):
    """utterances 0 and B - 1 against float64 on the CPU; asserts, and returns the figures"""
    leaf = logits.detach().requires_grad_(True)
    loss, stats = ops.rnnt_loss(leaf, el, labels, tl)
    (g,) = torch.autograd.grad(loss, leaf)
    torch.cuda.synchronize()
    out = {}
    eps = float(torch.finfo(torch.float32).eps)

    def restate(b, dtype):
        x = logits[b:b + 1].cpu().to(dtype).requires_grad_(True)
        ref, nll, valid = rr.rnnt_loss_ref(x, el[b:b + 1].cpu(), labels[b:b + 1].cpu(), tl[b:b + 1].cpu())
        (gr,) = torch.autograd.grad(ref, x)
        return float(nll[0].detach()), gr[0].double() / B, bool(valid[0])
    for b in (0, B - 1):
        # the bound of tests/test_gpu_rnnt.py: err <= K * floor + tiny, floor the restatement's own float32 run against its float64 run,
        # tiny = (T_b + U_b) * eps_fp32 * max |lp|: the rounding of the log-domain numbers the closed form holds
        nll, gr, valid = restate(b, torch.float64)
        nll32, gr32, _ = restate(b, torch.float32)
        Tb, Ub = int(el[b]), int(tl[b])
        lp_max = float(torch.log_softmax(logits[b, :Tb, :Ub + 1].cpu().double(), dim=-1).abs().max())
        tiny = (Tb + Ub) * eps * lp_max
        f_nll, f_g = abs(nll32 - nll) / abs(nll), float((gr32 - gr).norm() / gr.norm())
        e_nll = abs(float(stats['nll'][b]) - nll) / abs(nll)
        e_g = float((g[b].cpu().double() - gr).norm() / gr.norm())
        out['utt%d' % b] = {'nll': float(stats['nll'][b]), 'nll_ref': nll, 'nll_rel_err': e_nll, 'nll_floor': f_nll, 'grad_rel_err': e_g,
                            'grad_floor': f_g, 'tiny': tiny, 'K': CHECK_K, 'first_byte_offset': b * T * U1 * V * 4}
        assert valid and int(stats['valid'][b]) == 1, out
        assert e_nll <= CHECK_K * f_nll + tiny / abs(nll) and e_g <= CHECK_K * f_g + tiny, out
    del g, leaf
    return out


def loss_part(logits, el, labels, tl, iters):
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=DEV)    # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    leaf = logits.detach().requires_grad_(True)

    def fused(x=leaf):
        leaf.grad = None
        loss, _ = ops.rnnt_loss(x, el, labels, tl)
        if loss.requires_grad:
            ops.backward(loss)
        return loss
    nws = lib.otr_rnnt_workspace_floats(B, T, U1)
    ws, nll, loss1, dl = f32(nws), f32(B), f32(), f32(B, T, U1, V)
    valid = torch.empty((B,), dtype=torch.int32, device=DEV)

    def entry(grad=True):
        L.check(lib.otr_rnnt_loss(p(logits), V, p(labels), labels.stride(0), p(el), p(tl), B, T, U1, V, 0, None, p(loss1), p(nll), p(valid),
                                  p(dl) if grad else None, V, p(ws), nws, stream()), 'otr_rnnt_loss')
    r = {'fused_fwd_grad_ms': timed(fused, iters), 'fused_fwd_only_ms': timed(lambda: fused(logits), iters),
         'entry_fwd_grad_ms': timed(entry, iters), 'entry_fwd_only_ms': timed(lambda: entry(False), iters)}
    # the lattice and mean launches alone: the same entry on [B, T, U1, 2] logits, where the row pass reads 8 bytes a row.  What the
    # forward call takes beyond that is the row pass; what the call with a gradient takes beyond the forward call is the gradient pass
    two = torch.randn((B, T, U1, 2), device=DEV)
    lab2 = torch.ones_like(labels)

    def lattice():
        L.check(lib.otr_rnnt_loss(p(two), 2, p(lab2), lab2.stride(0), p(el), p(tl), B, T, U1, 2, 0, None, p(loss1), p(nll), p(valid),
                                  None, 2, p(ws), nws, stream()), 'otr_rnnt_loss')
    r['lattice_and_mean_ms'] = timed(lattice, iters)
    r['row_pass_ms'] = r['entry_fwd_only_ms'] - r['lattice_and_mean_ms']
    live_rows = int(((el.long()) * (tl.long() + 1)).sum())
    rows = B * T * U1
    fwd_bytes = live_rows * V * 4 + 3 * live_rows * 4
    grad_bytes = live_rows * V * 4 + rows * V * 4
    r.update(live_rows=live_rows, rows=rows, row_pass_traffic_mb=fwd_bytes / 1e6, grad_pass_traffic_mb=grad_bytes / 1e6,
             row_pass_floor_ms=fwd_bytes / HBM_BYTES_PER_S * 1e3, grad_pass_floor_ms=grad_bytes / HBM_BYTES_PER_S * 1e3)
    r['row_pass_over_floor'] = r['row_pass_ms'] / r['row_pass_floor_ms']
    r['grad_pass_ms'] = r['entry_fwd_grad_ms'] - r['entry_fwd_only_ms']
    r['grad_pass_over_floor'] = r['grad_pass_ms'] / r['grad_pass_floor_ms']
    del dl, ws
    # the composition from torch ops, at the largest batch that fits
    nb = B
    while nb >= 1:
        try:
            xs = logits[:nb].detach().clone().requires_grad_(True)

            def composed():
                xs.grad = None
                loss, _ = torch_rnnt(xs, el[:nb], labels[:nb], tl[:nb])
                loss.backward()
                return loss
            r['torch_composed_fwd_bwd_ms'] = timed(composed, max(2, iters // 3), warmup=1)
            want, nll_t = torch_rnnt(xs.detach(), el[:nb], labels[:nb], tl[:nb])
            got, st = ops.rnnt_loss(logits[:nb], el[:nb], labels[:nb], tl[:nb])
            r['torch_composed_batch'] = nb
            r['torch_composed_shape'] = 'the bench shape' if nb == B else 'B %d of %d: the largest that fits' % (nb, B)
            r['nll_max_rel_diff_vs_torch'] = float(((st['nll'] - nll_t).abs() / nll_t.abs()).max())
            if nb == B:
                r['torch_over_fused'] = r['torch_composed_fwd_bwd_ms'] / r['fused_fwd_grad_ms']
            else:
                sub = logits[:nb].detach().clone().requires_grad_(True)

                def fused_sub():
                    sub.grad = None
                    ops.backward(ops.rnnt_loss(sub, el[:nb], labels[:nb], tl[:nb])[0])
                r['fused_fwd_grad_ms_at_that_batch'] = timed(fused_sub, iters)
                r['torch_over_fused'] = r['torch_composed_fwd_bwd_ms'] / r['fused_fwd_grad_ms_at_that_batch']
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            nb //= 2
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}


def joint_part(el, tl, iters):
    g = torch.Generator(device=DEV).manual_seed(1)
    pe = torch.randn((B, T, J), generator=g, device=DEV).requires_grad_(True)
    pg = torch.randn((B, U1, J), generator=g, device=DEV).requires_grad_(True)
    dz = torch.randn((B, T, U1, J), generator=g, device=DEV)
    out = {}
    for mode in ('fp32', 'fp16'):
        ops.set_compute_dtype(mode)

        def fwd():
            with torch.no_grad():
                return ops.rnnt_joint(pe, pg, el, tl)

        def both():
            pe.grad = pg.grad = None
            ops.rnnt_joint(pe, pg, el, tl).backward(dz)
        n = B * T * U1 * J
        f, fb = timed(fwd, iters), timed(both, iters)
        fwd_bytes, bwd_bytes = n * (6 if mode != 'fp32' else 4), n * 16
        out[mode] = {'fwd_ms': round(f, 4), 'fwd_bwd_ms': round(fb, 4), 'bwd_ms': round(fb - f, 4), 'fwd_traffic_mb': fwd_bytes / 1e6,
                     'bwd_traffic_mb': bwd_bytes / 1e6, 'fwd_over_floor': round(f / (fwd_bytes / HBM_BYTES_PER_S * 1e3), 2),
                     'bwd_over_floor': round((fb - f) / (bwd_bytes / HBM_BYTES_PER_S * 1e3), 2)}
    ops.set_compute_dtype('bf16')
    return out


def step_part(a):
    ops.set_compute_dtype(a.mode)
    cfg = syn.c2_model(0.1)
    Vm = cfg['decoder']['vocab_size']
    params = {k: v for k, v in cfg.items() if k not in ('decoder', 'decoder_type')}
    params.update(vocab_size=Vm, joint_size=J, predictor=dict(embedding_size=256, hidden_size=512, num_layers=2, dropout=0.1))
    model = ota.TransducerModel(params)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).train()
    inputs, targets = syn.synthetic_batch(B, a.frames, 80, Vm, U1 - 1, seed=0)
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    state = {}

    def fwd():
        for p_ in model.parameters():
            p_.grad = None
        state['loss'] = model(inputs, targets)[0]

    def both():
        fwd()
        ops.backward(state['loss'])
    t_f = timed(fwd, a.iters)
    t_b = timed(both, a.iters)
    out = {'forward_ms': round(t_f, 3), 'backward_ms': round(t_b - t_f, 3), 'step_ms': round(t_b, 3), 'loss': float(state['loss'])}
    rec = ota.TransducerRecognizer(model, {i: str(i) for i in range(Vm)}, max_symbols=4, max_len=100)
    model.eval()
    tok = {}

    def decode():
        tok['out'] = rec.recognize_tokens(inputs['inputs'], inputs['mask'])
    out['greedy_decode_ms'] = round(timed(decode, max(2, a.iters // 3), warmup=1), 3)
    out['greedy_mean_tokens'] = round(float(tok['out'][1].float().mean()), 1)
    ops.set_compute_dtype('bf16')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--no-step', action='store_true', help='parts (0), (a) and (b) only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rnnt_bench needs a GPU')
    logits, el, labels, tl = make_batch()
    res = {'shape': {'B': B, 'T': T, 'U1': U1, 'V': V, 'J': J}, 'iters': a.iters, 'check': check_part(logits, el, labels, tl)}
    res['loss'] = loss_part(logits, el, labels, tl, a.iters)
    del logits
    torch.cuda.empty_cache()
    res['joint'] = joint_part(el, tl, a.iters)
    torch.cuda.empty_cache()
    if not a.no_step:
        res['step'] = dict(step_part(a), mode=a.mode, frames=a.frames, model='c2 encoder + LSTM predictor (E 256, H 512, 2 layers) + joint 512', B=B)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
