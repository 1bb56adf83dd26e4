"""MixSpeech benchmark (otr_mixspeech_mix, ops.ctc_loss_pair / otr_ctc_loss_pair, MixSpeechTraining).  Three parts, one JSON line:
 (a) the mix of a 32 x 1000 x 80 batch into its 16 pairs: otr_mixspeech_mix on preallocated buffers against the torch composition of
     the reference's trainer (a [P, T, F] tensor of lambda, two products, a sum, torch.max of masks and lengths) in the same run, with
     the bytes the call moves (read both utterances of a pair, write the pair) over its time.
 (b) ops.ctc_loss_pair forward + backward on [16, 250, 4233] logits with ~20 labels per utterance, against two ops.CTCLossFn calls
     combined with torch ops (lam * a + (1 - lam) * b, autograd adds the two gradients) on the same tensors.  The composition is timed
     twice: the pair call has to win by more than the two timings of the composition differ.  Losses and gradients are compared.
 (c) one C2 training step (forward + backward, eager, no optimizer) at B 32 in three forms on the same batch: MixSpeechTraining; the
     reference's form (mix with torch ops, model(mixed, t1) and model(mixed, t2), combine); the plain step.  ms and device launches per
     step (kernels and copies seen by torch.profiler in one step), without and with the CTC head.
Warm-up, then timed repeats with device events around groups of launches; medians.

    python tools/mixspeech_bench.py [--iters 20] [--frames 1000] [--mode fp16] [--no-step] [--out f.json]
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

LAM = 0.3
DEV = 'cuda'


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


def launches(fn):
    """device launches (kernels, copies, fills) of one fn() as torch.profiler sees them; None where the profiler reports none"""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                   # the count is a report, not a result: say why it is missing
        return 'profiler failed: %s' % type(e).__name__
    return n or None


def torch_mix(inputs, lam):
    """the reference's composition (trainer.py:163-182) on device tensors"""
    x = inputs['inputs']
    n = x.shape[0] // 2 * 2
    c = lam.unsqueeze(1).unsqueeze(1).repeat(n // 2, x.shape[1], x.shape[2])
    return {'inputs': x[0:n:2] * c + x[1:n:2] * (1 - c), 'mask': torch.max(inputs['mask'][0:n:2], inputs['mask'][1:n:2]),
            'inputs_length': torch.max(inputs['inputs_length'][0:n:2], inputs['inputs_length'][1:n:2])}


def mix_part(iters):
    B, T, F = 32, 1000, 80
    rng = np.random.default_rng(0)
    lens = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    lens[0] = T
    inputs, _ = syn.synthetic_batch(B, T, F, 100, 4, seed=0, lengths=[int(v) for v in lens])
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    lam = torch.tensor([LAM], dtype=torch.float32, device=DEV)
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    P = B // 2
    out = torch.empty((P, T, F), dtype=torch.float32, device=DEV)
    out_len = torch.empty((P,), dtype=torch.int32, device=DEV)
    mask = torch.empty((P, T), dtype=torch.bool, device=DEV)
    x, n = inputs['inputs'], inputs['inputs_length']

    def launch():
        L.check(lib.otr_mixspeech_mix(p(x), T * F, p(n), p(lam), B, T, F, p(out), p(out_len), p(mask),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_mixspeech_mix')
    t_kernel = timed(launch, iters, group=20)
    t_op = timed(lambda: ops.mixspeech_mix(x, n, lam), iters, group=20)
    t_torch = timed(lambda: torch_mix(inputs, lam), iters, group=5)
    t_torch_again = timed(lambda: torch_mix(inputs, lam), iters, group=5)
    launch()
    want = torch_mix(inputs, lam)
    torch.cuda.synchronize()
    assert torch.equal(out, want['inputs']) and torch.equal(mask, want['mask']) and torch.equal(out_len, want['inputs_length'])
    live = int(lens.sum())
    moved = (live * F + P * T * F) * 4 + P * T + (B + P) * 4          # live input frames read, every output cell written
    return {'shape': [B, T, F], 'kernel_ms': round(t_kernel, 4), 'ops_call_ms': round(t_op, 4), 'torch_ms': round(t_torch, 4),
            'torch_second_timing_ms': round(t_torch_again, 4), 'torch_over_kernel': round(t_torch / t_kernel, 2),
            'bytes_moved_mb': round(moved / 1e6, 2), 'kernel_gb_per_s': round(moved / t_kernel / 1e6, 1),
            'full_length_traffic_mb': round(3 * P * T * F * 4 / 1e6, 2), 'bit_equal_to_torch': True}


def ctc_part(iters):
    P, T, V, W = 16, 250, 4233, 24
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((P, T, V)).astype(np.float32)).to(DEV).requires_grad_(True)
    tl = rng.integers(16, W + 1, size=(2 * P,))
    tg = torch.from_numpy(rng.integers(1, V, size=(2 * P, W))).to(DEV)
    tl_d = torch.from_numpy(tl).to(DEV)
    il = torch.from_numpy(rng.integers(200, T + 1, size=(P,))).to(DEV)
    lam = torch.tensor([LAM], dtype=torch.float32, device=DEV)
    ta, tb, la, lb = tg[0::2], tg[1::2], tl_d[0::2].contiguous(), tl_d[1::2].contiguous()
    ta_c, tb_c = ta.contiguous(), tb.contiguous()          # CTCLossFn copies a strided view itself; keep that out of its time
    lam0, om0 = lam.reshape(()), 1 - lam.reshape(())
    state = {}

    def pair(backward=True, unit=False):
        x.grad = None
        state['loss'] = ops.ctc_loss_pair(x, ta, tb, il, la, lb, lam)[0]
        if backward:
            ops.backward(state['loss']) if unit else state['loss'].backward()

    def two_calls(backward=True):
        x.grad = None
        a = ops.CTCLossFn.apply(x, ta_c, il, la, 0)
        b = ops.CTCLossFn.apply(x, tb_c, il, lb, 0)
        state['loss'] = lam0 * a + om0 * b
        if backward:
            state['loss'].backward()
    t_two = timed(two_calls, iters, group=5)
    t_pair = timed(pair, iters, group=5)
    t_two_again = timed(two_calls, iters, group=5)
    t_pair_unit = timed(lambda: pair(unit=True), iters, group=5)
    with torch.no_grad():
        t_pair_fwd = timed(lambda: pair(False), iters, group=5)
        t_two_fwd = timed(lambda: two_calls(False), iters, group=5)
    pair()
    torch.cuda.synchronize()
    got_loss, got_grad = state['loss'].item(), x.grad.clone()
    two_calls()
    torch.cuda.synchronize()
    want_loss, want_grad = state['loss'].item(), x.grad
    gerr = float((got_grad - want_grad).norm() / want_grad.norm())
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss) and gerr < 1e-4, (got_loss, want_loss, gerr)
    spread = abs(t_two - t_two_again)
    return {'shape': [P, T, V], 'labels': [int(tl.min()), int(tl.max())], 'pair_fwd_bwd_ms': round(t_pair, 4),
            'two_calls_fwd_bwd_ms': round(t_two, 4), 'two_calls_second_timing_ms': round(t_two_again, 4),
            'two_calls_spread_ms': round(spread, 4), 'saved_ms': round(min(t_two, t_two_again) - t_pair, 4),
            'pair_faster_by_more_than_the_spread': bool(min(t_two, t_two_again) - t_pair > spread),
            'pair_over_two_calls': round(t_pair / t_two, 3), 'pair_fwd_bwd_unit_seed_ms': round(t_pair_unit, 4),
            'pair_fwd_only_ms': round(t_pair_fwd, 4), 'two_calls_fwd_only_ms': round(t_two_fwd, 4),
            'tensor_sized_transfers': {'pair': 6, 'two_calls': 15}, 'loss': got_loss, 'grad_rel_diff_vs_two_calls': gerr}


def step_part(a, ctc_weight):
    ops.set_compute_dtype(a.mode)
    cfg = syn.c2_model(0.1, ctc_weight=ctc_weight)
    V = cfg['decoder']['vocab_size']
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).train()
    inputs, targets = syn.synthetic_batch(32, a.frames, 80, V, 15, seed=0)
    inputs = {k: v.to(DEV) for k, v in inputs.items()}
    targets = {k: v.to(DEV) for k, v in targets.items()}
    wrap = ota.MixSpeechTraining(model).train()
    lam = wrap.set_lambda(LAM, inputs['inputs'].device)
    state = {}

    def reference_form():
        mixed = torch_mix(inputs, lam)
        loss_1, _ = model(mixed, {k: v[0::2] for k, v in targets.items()})
        loss_2, _ = model(mixed, {k: v[1::2] for k, v in targets.items()})
        return (torch.mean(lam * loss_1 + (1 - lam) * loss_2),)

    def step(fwd):
        def run():
            for p_ in model.parameters():
                p_.grad = None
            state['loss'] = fwd()[0]
            ops.backward(state['loss'])
        return run
    forms = {'mixspeech': step(lambda: wrap(inputs, targets, lam=lam)), 'reference_form': step(reference_form),
             'plain': step(lambda: model(inputs, targets))}
    out = {'ctc_weight': ctc_weight}
    for name, fn in forms.items():
        out[name + '_step_ms'] = round(timed(fn, a.iters), 3)
        out[name + '_loss'] = state['loss'].item()
    out['plain_second_timing_ms'] = round(timed(forms['plain'], a.iters), 3)
    for name, fn in forms.items():
        out[name + '_launches'] = launches(fn)
    out['mixspeech_over_reference_form'] = round(out['mixspeech_step_ms'] / out['reference_form_step_ms'], 3)
    out['mixspeech_over_plain'] = round(out['mixspeech_step_ms'] / out['plain_step_ms'], 3)
    out['mixspeech_faster_than_reference_form'] = bool(out['mixspeech_step_ms'] < out['reference_form_step_ms'])
    ops.set_compute_dtype('bf16')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--no-step', action='store_true', help='parts (a) and (b) only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mixspeech_bench needs a GPU')
    res = {'lam': LAM, 'iters': a.iters, 'mix': mix_part(a.iters), 'ctc_pair': ctc_part(a.iters)}
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
