"""Recurrent-LM training benchmark: egs/aishell/conf/rnnlm.yaml's model (V 4233, H 1024, 2 layers, tied, smoothing 0.1, dropout 0.1)
on random token batches with a PAD tail, T 40, batch 16 and 64, 16-bit mode (bf16 by default).  Times with device events after warm-up:
the forward pass, the backward pass, and the full train step through FlatDataParallel + FusedAdam (the yaml's Adam settings, clip 5);
reports tokens per second, the step-kernel launches per train step and the bytes each step kernel must read.  Prints one JSON line.

    python tools/rnnlm_train_bench.py [--batches 16,64] [--seq 40] [--mode bf16] [--iters 20] [--out f.json]
    python tools/rnnlm_train_bench.py --profile-once     # one train step, nothing else (run under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentransformer_amd import ops, synthetic as syn      # noqa: E402
from opentransformer_amd.dp import FlatDataParallel, FusedAdam      # noqa: E402
from opentransformer_amd.nn import PAD      # noqa: E402
from opentransformer_amd.recognize import LanguageModel      # noqa: E402


def make_batch(B, T, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    inp = torch.randint(1, V, (B, T), generator=g)
    tgt = torch.randint(1, V, (B, T), generator=g)
    for b in range(B):
        n = T - int(torch.randint(0, T // 4 + 1, (1,), generator=g))
        inp[b, n:] = PAD
        tgt[b, n:] = PAD
    return {'inputs': inp.cuda()}, {'targets': tgt.cuda()}


def step_read_bytes(B, H, es):
    """bytes one step launch must read (es: bytes per 16-bit / f32 operand element); 'per_wg' = one workgroup's share"""
    wg = H // 16
    fwd_w = 4 * H * H * es
    fwd = fwd_w + wg * B * H * es + B * 4 * H * 4 + 4 * H * 4 + B * H * 4            # W_hh pack, h_{t-1} per WG, gx, b_hh, c_{t-1}
    bwd = fwd_w + wg * B * 4 * H * es + B * H * 4 + B * 4 * H * 4 + 3 * B * H * 4      # pack, dG_{t+1} per WG, dy, act, c, c_{t-1}, dc
    return {'fwd_step': fwd, 'bwd_step': bwd, 'fwd_step_per_wg': fwd // wg, 'bwd_step_per_wg': bwd // wg, 'workgroups': wg}


def bench(B, T, mode, iters, warmup):
    ops.set_compute_dtype(mode)
    cfg = syn.rnn_lm_yaml_config()
    o = syn.RNN_LM_YAML_OPTIM
    lm = LanguageModel['rnn_lm'](cfg)
    syn.fill_state_dict_(lm.state_dict(), 1234)
    lm = lm.cuda().train()
    dp = FlatDataParallel(lm)
    opt = FusedAdam(dp, lr=o['lr'], betas=o['betas'], eps=o['eps'], weight_decay=o['weight_decay'], clip_grad=o['clip_grad'])
    inputs, targets = make_batch(B, T, cfg['vocab_size'])
    ntok = int((targets['targets'] != PAD).sum())

    def train_step(ev=None):
        dp.zero_grad(next_dropout_step=True)
        if ev:
            ev[0].record()
        loss, _ = dp(inputs, targets)
        if ev:
            ev[1].record()
        ops.backward(loss)
        if ev:
            ev[2].record()
        scale, _ = dp.all_reduce_gradients()
        opt.step(scale)
        if ev:
            ev[3].record()
        return loss

    for _ in range(warmup):
        train_step()
    torch.cuda.synchronize()
    fw, bw, st, losses = [], [], [], []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        s0 = torch.cuda.Event(enable_timing=True)
        s0.record()
        loss = train_step(ev)
        torch.cuda.synchronize()
        fw.append(ev[0].elapsed_time(ev[1]))
        bw.append(ev[1].elapsed_time(ev[2]))
        st.append(s0.elapsed_time(ev[3]))
        losses.append(loss.item())
    med = lambda x: float(np.median(x))      # noqa: E731
    H, nl = cfg['hidden_size'], cfg['num_layers']
    es = 4 if mode == 'fp32' else 2
    return {
        'batch': B, 'seq': T, 'mode': mode, 'fused_steps': ops.lstm_fused_applies(B, H),
        'fwd_ms': round(med(fw), 3), 'bwd_ms': round(med(bw), 3), 'step_ms': round(med(st), 3), 'step_ms_min': round(min(st), 3),
        'tokens_per_s': round(B * T / (med(st) * 1e-3)), 'target_tokens_per_s': round(ntok / (med(st) * 1e-3)),
        'step_kernel_launches': 2 * nl * T, 'pack_launches': 2 * nl,
        'fwd_us_per_layer_step': round(med(fw) * 1e3 / (nl * T), 2), 'bwd_us_per_layer_step': round(med(bw) * 1e3 / (nl * T), 2),
        'step_read_bytes': step_read_bytes(B, H, es), 'loss_first_last': [round(losses[0], 4), round(losses[-1], 4)],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--seq', type=int, default=40)
    ap.add_argument('--mode', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--profile-once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rnnlm_train_bench needs a GPU')
    sizes = [int(b) for b in a.batches.split(',')]
    if a.profile_once:
        r = bench(sizes[0], a.seq, a.mode, 1, 0)
        print(json.dumps({'profile_once': True, 'batch': sizes[0], 'seq': a.seq, 'mode': a.mode, 'step_ms': r['step_ms']}))
        return
    res = {'model': 'rnnlm.yaml (V 4233, H 1024, 2 layers, tied, dropout 0.1)', 'runs': [bench(B, a.seq, a.mode, a.iters, a.warmup) for B in sizes],
           'device': torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
