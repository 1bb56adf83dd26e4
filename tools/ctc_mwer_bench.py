"""MWER training of the CTC model, benchmark (ops.ctc_mwer_loss / otr_ctc_mwer_loss, CTCMWERTraining).  Two parts, one JSON line:
 (a) the loss alone on [32, 250, 4233] logits, N 4 and N 10 hypotheses of about 20 labels, with and without the reference term:
     ops.ctc_mwer_loss forward + gradient and forward only (the log-softmax included), the entry's own launches on a ready table of
     log-probabilities, against
       - the composed route's launches: N (+ 1) ops.CTCLossFn calls and the torch softmax ops over their [N] scores, forward + backward.
         CTCLossFn reports the batch mean, not the per-utterance likelihoods a posterior needs, so this route stands for the COST of
         composing the loss from what exists (N log-softmaxes, N dense slabs, autograd adding them up); its value is not the MWER loss;
       - the loss composed from torch.nn.functional.ctc_loss(reduction='none') per hypothesis, which is the MWER loss: its value and
         gradient are checked against the fused call's;
       - otr_ctc_loss alone (ops.CTCLossFn on the reference, and the entry on the ready table), forward + gradient;
       - its own minimum traffic -- one read of the [B, T, V] table for the log-softmax, one write of the gradient slab, the alpha
         tables -- at the 8 TB/s HBM figure of DESIGN.md.
 (b) the C2 encoder as a CTCModel, B 32, 1000 frames, eager: the CTCMWERTraining step (forward + backward, no optimizer) on the n-best
     of its own search, the search alone, and the plain CTCModel step on the same batch in the same run.
Warm-up, then timed repeats with device events; medians.

    python tools/ctc_mwer_bench.py [--iters 20] [--frames 1000] [--mode fp16] [--no-step] [--out f.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opentransformer_amd as ota                        # noqa: E402
from opentransformer_amd import _lib as L, ops, synthetic as syn          # noqa: E402

HBM_BYTES_PER_S = 8e12
B, T, V, LAB = 32, 250, 4233, 20
DEV = 'cuda'


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


def _edit(a, b):
    return ota.tools.edit_distance(a, b)


def loss_part(N, iters):
    rng = np.random.default_rng(N)
    logits = torch.from_numpy(rng.normal(size=(B, T, V)).astype(np.float32)).to(DEV)
    in_len = torch.from_numpy(rng.integers(T - 40, T + 1, size=B).astype(np.int32)).to(DEV)
    lens = rng.integers(LAB - 4, LAB + 5, size=B)
    W = int(lens.max())
    refs = np.zeros((B, W), np.int64)
    hyps = np.zeros((B, N, W), np.int64)
    errors = np.zeros((B, N), np.int32)
    for b in range(B):
        truth = rng.integers(1, V, size=lens[b])
        refs[b, :lens[b]] = truth
        for n in range(N):                                 # the recipe of tests/ctc_mwer_cases.py: 1 + n % 3 substitutions
            h = truth.copy()
            if n:
                for i in rng.choice(lens[b], size=1 + n % 3, replace=False):
                    h[i] = 1 + (h[i] - 1 + rng.integers(1, V - 1)) % (V - 1)
            hyps[b, n, :lens[b]] = h
            errors[b, n] = _edit(truth.tolist(), h.tolist())
    ref_d, hyp_d, err_d = torch.from_numpy(refs).to(DEV), torch.from_numpy(hyps).to(DEV), torch.from_numpy(errors).to(DEV)
    ref_len = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    hyp_len = ref_len.unsqueeze(1).repeat(1, N).contiguous()
    leaf = logits.clone().requires_grad_(True)
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=DEV)    # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    lp = ops.log_softmax(logits)
    out = {}
    for tag, with_ref, w in (('noref', False, 0.0), ('ref', True, 0.3)):
        kw = dict(ref=ref_d, ref_len=ref_len, ctc_weight=w) if with_ref else {}

        def fused(x=leaf):
            leaf.grad = None
            loss, _ = ops.ctc_mwer_loss(x, in_len, hyp_d, hyp_len, err_d, **kw)
            if loss.requires_grad:
                ops.backward(loss)
            return loss
        loss3, seq, post, utt, nll, dl = f32(3), f32(B, N), f32(B, N), f32(B), f32(B), f32(B, T, V)
        nws = lib.otr_ctc_mwer_workspace_floats(B, N, T, W)
        ws = f32(nws)

        def entry(grad=True):
            L.check(lib.otr_ctc_mwer_loss(p(lp), p(in_len), p(hyp_d), W, p(hyp_len), p(err_d), p(ref_d) if with_ref else None,
                                          W if with_ref else 0, p(ref_len) if with_ref else None, w, 1.0, None, B, N, T, V, W, 0, p(loss3),
                                          p(seq), p(post), p(utt), p(nll), p(dl) if grad else None, p(ws), nws, stream()), 'otr_ctc_mwer_loss')

        def composed_fn():
            """the cost of the composition from ops.CTCLossFn (see the module docstring: not the MWER value)"""
            leaf.grad = None
            s = torch.stack([-ops.CTCLossFn.apply(leaf, hyp_d[:, n].contiguous(), in_len, hyp_len[:, n].contiguous(), 0) for n in range(N)])
            total = (torch.softmax(s, dim=0) * err_d.float().mean(dim=0)).sum()
            if with_ref:
                total = total + w * ops.CTCLossFn.apply(leaf, ref_d, in_len, ref_len, 0)
            total.backward()

        def composed_torch(x=leaf):
            """the MWER loss from F.ctc_loss(reduction='none') per hypothesis"""
            leaf.grad = None
            lpt = F.log_softmax(x, dim=-1).transpose(0, 1)
            il = in_len.long()
            s = torch.stack([-F.ctc_loss(lpt, hyp_d[:, n], il, hyp_len[:, n].long(), blank=0, reduction='none') for n in range(N)], dim=1)
            total = (torch.softmax(s, dim=1) * err_d.float()).sum(dim=1).mean()
            if with_ref:
                nl = F.ctc_loss(lpt, ref_d, il, ref_len.long(), blank=0, reduction='none', zero_infinity=True)
                total = total + w * (nl / ref_len.clamp(min=1)).mean()
            if total.requires_grad:
                total.backward()
            return total
        r = {'fused_fwd_grad_ms': timed(fused, iters), 'fused_fwd_only_ms': timed(lambda: fused(logits), iters),
             'entry_fwd_grad_ms': timed(entry, iters), 'entry_fwd_only_ms': timed(lambda: entry(False), iters),
             'composed_ctclossfn_fwd_bwd_ms': timed(composed_fn, iters)}
        try:
            r['composed_torch_fwd_bwd_ms'] = timed(composed_torch, iters)
            want = composed_torch()
            g_want = leaf.grad.clone()
            got = fused()
            torch.cuda.synchronize()
            got, want = float(got.detach()), float(want.detach())
            r['loss'] = got
            r['loss_diff_vs_torch'] = abs(got - want)
            r['grad_rel_diff_vs_torch'] = float((leaf.grad - g_want).abs().max() / g_want.abs().max())
            assert r['loss_diff_vs_torch'] < 1e-3 * max(1.0, abs(want)) and r['grad_rel_diff_vs_torch'] < 1e-2, r
            r['torch_over_fused'] = r['composed_torch_fwd_bwd_ms'] / r['fused_fwd_grad_ms']
        except RuntimeError as e:                          # a torch build without a device ctc_loss: the comparison is left out
            r['composed_torch'] = 'not run: %s' % str(e).splitlines()[0]
        traffic = (2 * B * T * V + (N + (1 if with_ref else 0)) * B * T * (2 * W + 1)) * 4
        floor_ms = traffic / HBM_BYTES_PER_S * 1e3
        r.update(composed_over_fused=r['composed_ctclossfn_fwd_bwd_ms'] / r['fused_fwd_grad_ms'],
                 fused_not_slower_than_composed=bool(r['fused_fwd_grad_ms'] <= r['composed_ctclossfn_fwd_bwd_ms']),
                 traffic_mb=traffic / 1e6, traffic_floor_ms_at_8TBps=floor_ms, fused_over_floor=r['fused_fwd_grad_ms'] / floor_ms)
        out[tag] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    # otr_ctc_loss alone on the same tensors
    ws1, nll1, loss1, dl1 = f32(B, T, 2 * W + 1), f32(B), f32(), f32(B, T, V)

    def ctc_entry():
        L.check(lib.otr_ctc_loss(p(lp), p(ref_d), W, p(in_len), p(ref_len), B, T, V, W, 0, p(ws1), p(nll1), p(loss1), p(dl1), stream()),
                'otr_ctc_loss')

    def ctc_fn():
        leaf.grad = None
        ops.backward(ops.CTCLossFn.apply(leaf, ref_d, in_len, ref_len, 0))
    out['ctc_loss_alone'] = {'entry_fwd_grad_ms': round(timed(ctc_entry, iters), 4), 'CTCLossFn_fwd_bwd_ms': round(timed(ctc_fn, iters), 4),
                             'log_softmax_ms': round(timed(lambda: ops.log_softmax(logits), iters), 4)}
    return out


def step_part(a, N=4):
    ops.set_compute_dtype(a.mode)
    cfg = syn.c2_model(0.1)
    Vm = cfg['decoder']['vocab_size']
    model = ota.CTCModel(dict(cfg, vocab_size=Vm))
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).train()
    inputs, targets = syn.synthetic_batch(B, a.frames, 80, Vm, 15, seed=0)
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    wrap = ota.CTCMWERTraining(model, nbest=N)
    state = {}

    def clear():
        for p_ in model.parameters():
            p_.grad = None

    def mwer_fwd():
        clear()
        state['loss'] = wrap(inputs, targets, hyps=state.get('hyps'))[0]

    def ctc_fwd():
        clear()
        state['loss'] = model(inputs, targets)[0]

    def split(fwd):
        def both():
            fwd()
            ops.backward(state['loss'])
        t_fwd = timed(fwd, a.iters)
        t_both = timed(both, a.iters)
        return t_fwd, t_both - t_fwd, t_both
    out = {'search_ms': round(timed(lambda: wrap.search(inputs['inputs'], inputs['mask']), a.iters), 3)}
    tokens, lengths, dead = wrap.search(inputs['inputs'], inputs['mask'])
    out.update(search_mean_hyp_labels=round(float(lengths.float().mean()), 1), search_dead_slots=int(dead.sum()),
               search_slots_over_127_labels=int((lengths > 127).sum()), search_row_width=int(tokens.shape[2]))
    f, b, t = split(mwer_fwd)                              # hyps=None: the search runs inside the step
    out.update(mwer_step_with_search_forward_ms=round(f, 3), mwer_step_with_search_backward_ms=round(b, 3), mwer_step_with_search_ms=round(t, 3))
    state['hyps'] = (tokens, lengths)
    f, b, t = split(mwer_fwd)
    out.update(mwer_forward_ms=round(f, 3), mwer_backward_ms=round(b, 3), mwer_step_ms=round(t, 3))
    rec = []
    ops.set_kernel_timer(rec)
    try:
        for _ in range(5):
            mwer_fwd()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    out['mwer_loss_launches_ms'] = round(float(np.median([e0.elapsed_time(e1) for name, _, e0, e1, _ in rec if name.startswith('ctc_mwer_loss')])), 4)
    f, b, t = split(ctc_fwd)
    out.update(ctc_forward_ms=round(f, 3), ctc_backward_ms=round(b, 3), ctc_step_ms=round(t, 3))
    out['mwer_step_over_ctc_step'] = round(out['mwer_step_ms'] / out['ctc_step_ms'], 3)
    out['mwer_step_with_search_over_ctc_step'] = round(out['mwer_step_with_search_ms'] / out['ctc_step_ms'], 3)
    ops.set_compute_dtype('bf16')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--no-step', action='store_true', help='part (a) only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ctc_mwer_bench needs a GPU')
    res = {'shape': {'B': B, 'T': T, 'V': V, 'labels': LAB}, 'iters': a.iters, 'loss': {'N%d' % n: loss_part(n, a.iters) for n in (4, 10)}}
    if not a.no_step:
        res['step'] = dict(step_part(a), mode=a.mode, frames=a.frames, model='c2 encoder + CTC head', B=B, N=4)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
