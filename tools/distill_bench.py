"""Knowledge-distillation benchmark (ops.distill_loss / otr_distill_loss, DistillTraining).  Two parts, one JSON line:
 (a) otr_distill_loss forward + gradient on preallocated buffers at the CTC-head shape (32 x 250 rows, V 4233 in rows of 4240) and the
     decoder shape (32 x 15 rows, V 4234 in rows of 4240), against a dense teacher and against a top-40 teacher; against the same loss
     composed from torch ops (log_softmax of both, exp, masked sum; autograd for the gradient) on the same logits in the same run; and
     as a multiple of the time of the call's own minimum traffic -- read the student, read the teacher, write the gradient -- at the
     8 TB/s HBM figure of DESIGN.md.  The composed route's loss and gradient are checked against the kernel's.
 (b) one C2 DistillTraining step (forward + backward, eager, no optimizer) at B 32 with a teacher of the student's size: online (the
     teacher pass inside the step), offline from stored dense logits and offline from stored top-40 pairs, beside the plain step of the
     same model on the same batch in the same run; without and with the CTC head.
Warm-up, then timed repeats with device events around groups of launches; medians.

    python tools/distill_bench.py [--iters 20] [--frames 1000] [--mode fp16] [--no-step] [--out f.json]
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
SHAPES = {'ctc_head': (32, 250, 4233, 4240), 'decoder': (32, 15, 4234, 4240)}
K, TAU = 40, 2.0


def timed(fn, iters, warmup=3, group=1):
    """median time of one fn() in ms; `group` calls share one pair of events so that a short call is not a measurement of the events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(group):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / group)
    return float(np.median(ts))


def composed(s, t_logits, live):
    """the dense loss from torch ops; t_logits holds -inf off the list for a sparse teacher"""
    lp = torch.log_softmax(s / TAU, dim=-1)
    lq = torch.log_softmax(t_logits / TAU, dim=-1)
    q = lq.exp()
    kl = torch.where(q > 0, q * (lq - lp), torch.zeros_like(q)).sum(-1)
    return TAU * TAU * torch.where(live, kl, torch.zeros_like(kl)).sum() / live.sum()


def kernel_part(name, iters):
    Bn, Tn, V, LD = SHAPES[name]
    R = Bn * Tn
    rng = np.random.default_rng(0)
    dev = 'cuda'
    s_full = torch.from_numpy((rng.normal(size=(R, LD)) * 4).astype(np.float32)).to(dev)
    t_full = s_full + torch.from_numpy((rng.normal(size=(R, LD)) * 2).astype(np.float32)).to(dev)
    lens = rng.integers(Tn // 2, Tn + 1, size=Bn).astype(np.int32)
    lengths = torch.from_numpy(lens).to(dev)
    live = (torch.arange(Tn, device=dev).unsqueeze(0) < lengths.unsqueeze(1))
    s_view, t_view = s_full[:, :V].view(Bn, Tn, V), t_full[:, :V].view(Bn, Tn, V)
    top_val, top_idx = ops.topk_rows(t_view, torch.full_like(lengths, Tn), K)
    t_masked = torch.full((Bn, Tn, V), float('-inf'), device=dev).scatter_(-1, top_idx.long(), top_val)
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)    # noqa: E731
    loss, row_kl, dl = f32(1), f32(R), f32(R, LD)
    nws = lib.otr_distill_workspace_floats(Bn, Tn)
    ws = f32(nws)

    def launch(sparse, grad=True):
        L.check(lib.otr_distill_loss(p(s_full), LD, None if sparse else p(t_full), 0 if sparse else LD, p(top_val) if sparse else None,
                                     p(top_idx) if sparse else None, K if sparse else 0, p(lengths), Bn, Tn, V, TAU, None, p(loss), p(row_kl),
                                     p(dl) if grad else None, LD, p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                'otr_distill_loss')
    leaf = s_full.clone().requires_grad_(True)

    def torch_route(teacher):
        leaf.grad = None
        composed(leaf[:, :V].view(Bn, Tn, V), teacher, live).backward()
    live_rows = int(lens.sum())
    out = {'rows': R, 'live_rows': live_rows, 'V': V, 'ld': LD}
    group = 20 if R < 2000 else 5
    for tag, sparse, teacher in (('dense', False, t_view), ('top%d' % K, True, t_masked)):
        t_kernel = timed(lambda: launch(sparse), iters, group=group)
        t_fwd = timed(lambda: launch(sparse, False), iters, group=group)
        t_torch = timed(lambda: torch_route(teacher), iters)
        with torch.no_grad():
            t_torch_fwd = timed(lambda: composed(s_view, teacher, live), iters)
            want = composed(s_view, teacher, live)
        launch(sparse)
        torch_route(teacher)
        torch.cuda.synchronize()
        assert abs(float(loss) - float(want)) < 1e-4 * max(1.0, abs(float(want))), (tag, float(loss), float(want))
        gerr = float((dl - leaf.grad).abs().max() / leaf.grad.abs().max())
        assert gerr < 1e-4, (tag, gerr)
        # the least the call could move: the live rows of the student and of the teacher once, the whole gradient once
        traffic = (live_rows * V + (live_rows * 2 * K if sparse else live_rows * V) + R * LD) * 4
        floor_ms = traffic / HBM_BYTES_PER_S * 1e3
        out[tag] = {'kernel_fwd_grad_ms': round(t_kernel, 4), 'kernel_fwd_only_ms': round(t_fwd, 4), 'torch_fwd_grad_ms': round(t_torch, 4),
                    'torch_fwd_only_ms': round(t_torch_fwd, 4), 'torch_over_kernel': round(t_torch / t_kernel, 2),
                    'kernel_not_slower_than_torch': bool(t_kernel <= t_torch), 'min_traffic_mb': round(traffic / 1e6, 2),
                    'min_traffic_ms_at_8TBps': round(floor_ms, 4), 'kernel_over_min_traffic': round(t_kernel / floor_ms, 2),
                    'loss': float(loss), 'grad_rel_diff_vs_torch': gerr}
    return out


def step_part(a, ctc_weight):
    dev = 'cuda'
    ops.set_compute_dtype(a.mode)
    cfg = syn.c2_model(0.1, ctc_weight=ctc_weight)
    V = cfg['decoder']['vocab_size']
    models = []
    for seed in (1234, 4321):
        m = ota.SpeechToText(cfg)
        syn.fill_state_dict_(m.state_dict(), seed)
        models.append(m.to(dev))
    model, teacher = models[0].train(), models[1]
    inputs, targets = syn.synthetic_batch(32, a.frames, 80, V, 15, seed=0)
    inputs = {k: v.to(dev) for k, v in inputs.items()}
    targets = {k: v.to(dev) for k, v in targets.items()}
    online = ota.DistillTraining(model, teacher, temperature=TAU)
    dense = online.teacher_outputs(inputs, targets)
    pairs = ota.DistillTraining(model, teacher, temperature=TAU, topk=K).teacher_outputs(inputs, targets)
    offline = ota.DistillTraining(model, None, temperature=TAU)
    state = {}

    def step(fwd):
        def run():
            for p_ in model.parameters():
                p_.grad = None
            state['loss'] = fwd()[0]
            ops.backward(state['loss'])
        return run
    out = {'ctc_weight': ctc_weight,
           'plain_step_ms': round(timed(step(lambda: model(inputs, targets)), a.iters), 3),
           'teacher_pass_ms': round(timed(lambda: online.teacher_outputs(inputs, targets), a.iters), 3),
           'distill_online_step_ms': round(timed(step(lambda: online(inputs, targets)), a.iters), 3),
           'distill_offline_dense_step_ms': round(timed(step(lambda: offline(inputs, targets, teacher_out=dense)), a.iters), 3),
           'distill_offline_top%d_step_ms' % K: round(timed(step(lambda: offline(inputs, targets, teacher_out=pairs)), a.iters), 3)}
    rec = []
    ops.set_kernel_timer(rec)
    try:
        for _ in range(5):
            step(lambda: offline(inputs, targets, teacher_out=dense))()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    for name in sorted({n for n, _, _, _, _ in rec if n.startswith('distill_loss')}):
        out['launches_ms ' + name] = round(float(np.median([e0.elapsed_time(e1) for n, _, e0, e1, _ in rec if n == name])), 4)
    for k in ('distill_online_step_ms', 'distill_offline_dense_step_ms', 'distill_offline_top%d_step_ms' % K):
        out[k.replace('_ms', '_over_plain')] = round(out[k] / out['plain_step_ms'], 3)
    out['stored_mb_per_batch'] = {'dense': round(sum(v.numel() for v in dense.values()) * 4 / 1e6, 1),
                                  'top%d' % K: round(sum(v.numel() + i.numel() for v, i in pairs.values()) * 4 / 1e6, 2)}
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
        raise SystemExit('distill_bench needs a GPU')
    res = {'tau': TAU, 'K': K, 'iters': a.iters, 'kernel': {name: kernel_part(name, a.iters) for name in SHAPES}}
    if not a.no_step:
        res['step'] = [dict(step_part(a, w), mode=a.mode, frames=a.frames, model='c2', B=32) for w in (0.0, 0.3)]
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
