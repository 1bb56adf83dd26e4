#!/usr/bin/env python3
"""bench.py -- utterances/sec of the otrans speech-transformer TRAIN step on MI355X.

Workload (BASELINE.json configs[1]): egs/aishell/conf/transformer_baseline.yaml with
frontend.input_size 80, residual_dropout 0.1, synthetic 80-d fbank x 1000 frames, 15 decoder rows,
B = 32 utterances per GPU, 16-bit MFMA operands / fp32 accumulate.  One step = zero grads, forward, backward,
ONE gradient all-reduce (N>1), clip + Adam + Noam update: nothing is skipped in the timed region.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

--dump-outputs DIR writes what the last of the K timed steps computed as DIR/<name>.npy (train: loss.npy, params.npy and
grads.npy -- a fixed seeded sample of 2^20 of the updated parameters and of their gradients --, optimizer.npy; decode: hyps.npy,
scores.npy).  The inputs and weights are seeded, so two builds run with the same flags compare output for output -- within a
tolerance: two runs of one build already differ in the last bits (loss ~1e-6 relative, parameters ~2e-7).

N > 1 without a torchrun environment re-launches itself as `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>` (one rank per GPU over RCCL); under
torchrun it reads RANK / LOCAL_RANK / WORLD_SIZE as usual.

A plain run sets up, warms up, times the K steps, writes its outputs (--dump-outputs) and prints ONE JSON line (rank 0):
metric, value, unit, higher_is_better, dtype, ms_per_step and the configuration.  --full also measures, after the timed steps
(--task decode: the CPU baseline alone),
  windows       five further windows of K steps, timed like the timed region;
  step_breakdown  forward + backward against all-reduce + optimizer, from events; at N > 1 also the collective on its own and
                the step without collectives and with a bf16 gradient payload;
  roofline      the kernel with the largest share of the training step (launches x duration; today the fused FFN backward),
                its launch re-timed back to back inside a hipGraph with events on the launch stream, FLOPs / duration against
                the 16-bit MFMA peak, HBM traffic and MFMA-busy share from the committed --pmc passes; `roofline_kernels`
                lists the other hot launches of the same instrumented step (incl. the HBM-bound weight-gradient launch);
  bf16          the same workload timed in bf16 mode (BASELINE configs[1] names bf16; the headline runs fp16, see below);
  cpu_baseline  the CPU oracle (a port: /root/reference does not exist on the GPU box) on the host cores, B=32, best of
                16 / 32 / 64 torch threads.

Compute mode: fp16 MFMA operands by default.  bf16 operands (8 mantissa bits) put the logits 4.2e-3 from the fp32
reference, fp16 (11 bits) 5.4e-4 -- inside the north-star's 1e-3 -- at the same MFMA rate (tests/test_gpu_headline.py,
tools/precision_study.py); gradients are loss-scaled on the device (dynamic, inside otr_optimizer_step).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from opentransformer_amd import synthetic as syn          # noqa: E402

PEAK_16BIT_TFLOPS = 2500.0    # MI355X dense bf16 / fp16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32, help='utterances per GPU')
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'],
                    help='MFMA operand type: fp16 (default; logits within 1e-3 of the fp32 reference), bf16, or fp32 (exact-fp32 MFMA)')
    ap.add_argument('--model', default='transformer', choices=['transformer', 'conformer'],
                    help='transformer = BASELINE configs[1] (the metric); conformer = configs[3] (informative)')
    ap.add_argument('--task', default='train', choices=['train', 'decode'],
                    help='train = the metric (BASELINE configs[1]); decode = configs[4] (C5): batch beam search + LM fusion, one GPU')
    ap.add_argument('--no-graph', action='store_true', help='launch eagerly instead of replaying a hipGraph')
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps, also measure the windows, step breakdown, roofline, bf16 line and CPU baseline '
                         '(decode: the CPU baseline); a plain run times the contract region alone')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-extras', action='store_true', help='with --full: no windows, step breakdown, roofline or bf16 line')
    ap.add_argument('--no-bf16-line', action='store_true', help='with --full: skip the secondary bf16 measurement of the same workload')
    ap.add_argument('--overlap', default='auto', choices=['auto', 'on', 'off'],
                    help='off = ONE gradient all-reduce per step behind the backward pass (what north_star states; the form at N = 1).  '
                         'on = staged step: the backward pass is cut at the encoder / decoder boundary into two hipGraphs, and between '
                         'their replays the all-reduce of the decoder group (37 %% of the gradient bytes) starts on a side stream and runs '
                         'beside the encoder backward; the collectives themselves are never captured.  auto (N > 1) = MEASURE both forms '
                         'for a few untimed steps in this invocation and run the contract region on the faster one; off when N = 1')
    ap.add_argument('--dropout', type=float, default=0.1, help='residual_dropout of the workload (the shipped yaml: 0.1; other values are experiments, not the metric)')
    ap.add_argument('--calib-steps', type=int, default=8, help='steps per form of the --overlap auto measurement (N > 1)')
    ap.add_argument('--opt-in-graph', default='on', choices=['on', 'off'],
                    help='N = 1: capture the optimizer launches in the step graph too (on) or issue them eagerly behind the replay (off)')
    ap.add_argument('--cpu-threads', type=int, default=0, help='torch threads of the CPU baseline (0 = best of 16 / 32 / 64)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, '
                         'a fixed seeded sample of the parameter-sized outputs): two builds run with the same flags compare output for output')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    return args


DUMP_SAMPLE = 1 << 20       # elements kept of each parameter-sized output (4 MB in float32; the AISHELL model has 36.5 M parameters)


def dump_outputs(out_dir, arrays):
    """write {name: float32 / float64 array} as out_dir/<name>.npy"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + '.npy'), a)


def train_step_outputs(run, loss):
    """what a caller of the timed train step holds after it: the loss of the step, and the model's parameters (updated by the
    step's optimizer) and their gradients as the step left them in .grad (loss-scaled in fp16 mode), in model.parameters() order --
    the two parameter-sized outputs as the same fixed, seeded sample of DUMP_SAMPLE positions on every run"""
    import numpy as np
    params = run['dp'].params
    with torch.no_grad():
        flat_p = torch.cat([p.detach().reshape(-1) for p in params]).float()
        flat_g = torch.cat([p.grad.detach().reshape(-1) for p in params]).float()
    n = flat_p.numel()
    if n > DUMP_SAMPLE:
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))).to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    st = run['opt'].stats()
    return {'loss': np.array([loss], dtype=np.float64),
            'params': flat_p.cpu().numpy(), 'grads': flat_g.cpu().numpy(),
            'optimizer': np.array([st[k] for k in ('step', 'lr', 'grad_sqnorm', 'loss_scale', 'skipped', 'faults')], dtype=np.float64)}


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` (N > 1) outside torchrun: become N ranks on this node."""
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus:
        print('bench.py: --gpus %d requested but only %d GPU(s) are visible' % (args.gpus, n_dev), file=sys.stderr)
        sys.exit(2)
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def cpu_baseline(args):
    """The CPU oracle (oracle/otrans_oracle.py: a restatement of the reference path, pinned to the real reference by
    tests/test_oracle_golden.py; kind 'port' because /root/reference is not present on the GPU box) timed on the host
    cores: train fwd+bwd, fp32, same model config, B = 32 (the bench batch), the best of 16 / 32 / 64 torch threads
    (torch's CPU kernels stop scaling long before a 256-thread host is full: 0.24 s / iteration at 16 threads, 0.80 s at 64,
    173 s at 256 for B=4 on the r02 box), median of >= 5 iterations at the best setting."""
    from oracle import otrans_oracle as orc
    from tests import helpers as H
    host = os.cpu_count() or 1
    cfg = syn.c2_model(0.0)
    parts = H.require_grad(H.filled_state(cfg))
    flat = [t for sd in parts.values() for t in sd.values()]
    inputs, targets = syn.synthetic_batch(args.batch, args.frames, 80, 4234, 15, seed=0)

    def one():
        for t in flat:
            t.grad = None
        t0 = time.perf_counter()
        loss, _ = orc.speech2text_forward(parts, cfg, inputs, targets)
        loss.backward()
        return time.perf_counter() - t0

    tried, best = {}, None
    for threads in ([args.cpu_threads] if args.cpu_threads else [t for t in (16, 32, 64) if t <= host] or [host]):
        torch.set_num_threads(threads)
        one()                                                   # warm-up (allocator, thread pool)
        times = [one(), one()]
        if best is None or sorted(times)[0] < 1.25 * best[1]:   # worth finishing: within reach of the best so far
            times += [one() for _ in range(3)]
        med = sorted(times)[len(times) // 2]
        tried[threads] = {'utt_per_s': args.batch / med, 'iters': len(times)}
        if len(times) >= 5 and (best is None or med < best[1]):
            best = (threads, med)
    threads, med = best
    ratio = None
    try:        # the port's speed relative to the REAL reference, measured where /root/reference exists (tools/cpu_ref_vs_port.py)
        rr = json.load(open(os.path.join(ROOT, 'profiles', 'r04_cpu_ref_vs_port.json')))
        ratio = {'same_config_dropout_0': rr['reference_dropout_0.0']['port_over_reference'],
                 'reference_with_yaml_dropout_0.1': rr['reference_dropout_0.1']['port_over_reference'],
                 'judge_r03': rr['judge_r03']['port_over_reference'],
                 'note': 'port utt/s divided by reference utt/s on the SAME cores (8 threads, B=4, build container): the port is this much '
                         'FASTER than the reference, so the baseline above is generous to the CPU; value / ratio estimates the reference'}
    except Exception:                                          # noqa: BLE001
        pass
    return {'value': args.batch / med, 'unit': 'utterances/s', 'cores': threads, 'host_cores': host, 'kind': 'port',
            'port_over_reference': ratio, 'by_threads': tried,
            'sample': 'CPU oracle (port of the reference path; the reference tree is absent on the GPU box) fwd+bwd fp32, B=%d x '
                      '%d frames, median of 5 iterations (1 warm-up) at the best of %s torch threads on a %d-core host'
                      % (args.batch, args.frames, '/'.join(str(t) for t in tried), host)}


def replay_dominant(ops, name, mode):
    """Accurate launch duration of the dominant kernel: its launch is re-issued 10x back to back on the operands of the
    last step inside ONE hipGraph (no host gaps between launches) and timed with events on the launch stream."""
    if name != 'linear_wgrad_grouped':
        return None
    w, _ = ops._wq.get('last', ([], []))
    if not w:
        return None
    # the dominant LAUNCH is the 256-wide kernel over the longest-contraction group (the encoder's 48 wide problems, the
    # decoder's cross-attention key/value slices and the frontend Linear: M = B x T'); the short decoder problems run in a
    # second, much smaller launch of the same kernel
    m_max = max(wi[0].shape[0] for wi in w)
    w = [wi for wi in w if wi[0].shape[0] == m_max and wi[0].dtype == wi[1].dtype and wi[0].dtype != torch.float32]
    if not w:
        return None
    flops = sum(2.0 * wi[0].shape[0] * wi[0].shape[1] * wi[1].shape[1] for wi in w)
    nbytes = sum(wi[0].shape[0] * wi[0].shape[1] * wi[0].element_size() + wi[1].numel() * wi[1].element_size() + 2 * wi[2].numel() * 4
                 for wi in w)

    def run():
        ops._wq['w'], ops._wq['b'] = list(w), []
        ops.flush_weight_grads()
    ops._wq['keep_last'] = False
    n = 10
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            for _ in range(n):
                run()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return {'ms': e0.elapsed_time(e1) / n, 'flops': flops, 'bytes': nbytes, 'problems': len(w), 'rows': m_max}
    except Exception:                                          # noqa: BLE001
        return None


def instrumented_step(ops, fwd_bwd, mode):
    """One EAGER training step with ops' kernel timer installed: every hot launch is bracketed by events on the launch
    stream.  Returns {kernel name: {avg_launch_ms, launches, total_ms, achieved, frac, ...}} for this step."""
    rec = []
    ops._wq['keep_last'] = True            # keep the grouped weight-gradient operands of the pass for replay_dominant()
    for _ in range(2):                    # the first pass warms caches / allocator, the second is kept
        rec.clear()
        ops.set_kernel_timer(rec)
        try:
            fwd_bwd()
            torch.cuda.synchronize()
        finally:
            ops.set_kernel_timer(None)
    peak = PEAK_F32_TFLOPS if mode == 'fp32' else PEAK_16BIT_TFLOPS
    agg = {}
    for name, meta, e0, e1, call in rec:
        a = agg.setdefault(name, {'launches': 0, 'total_ms': 0.0, 'flops': 0.0, 'bytes': 0.0})
        a.setdefault('calls', []).append(call)    # every launch of this name in the step: replay_call() re-times them without host gaps
        a['launches'] += 1
        a['total_ms'] += e0.elapsed_time(e1)
        a['flops'] += (meta or {}).get('flops', 0.0)
        a['bytes'] += (meta or {}).get('bytes', 0.0)
        if meta and 'problems' in meta:
            a['problems'] = meta['problems']
    for a in agg.values():
        a['avg_launch_ms'] = a['total_ms'] / a['launches']
        a['achieved'] = a['flops'] / (a['total_ms'] * 1e-3) / 1e12 if a['total_ms'] > 0 else 0.0    # TFLOP/s
        a['frac'] = a['achieved'] / peak
        a['algorithmic_bytes_per_launch'] = a.pop('bytes') / a['launches']
        a['flops_per_launch'] = a.pop('flops') / a['launches']
    return agg


KERNEL_LABEL = {
    'linear_wgrad_grouped': 'wgrad256_kernel (weight + bias gradients of every wide Linear of the backward pass: one persistent 256x256-tile launch per row count; the rest on gemm_grouped_kernel)',
    'proj_ln_fwd': 'proj_ln_fwd_kernel (attention output projection + bias + dropout + residual + LayerNorm, row-block fused)',
    'ln_bwd_proj': 'ln_bwd_proj_kernel (LayerNorm backward + input gradient of the output projection, row-block fused)',
    'ffn_ln_fwd': 'ffn_ln_fwd_kernel (w_1 + GLU + w_2 + bias + dropout + residual + LayerNorm, row-block fused)',
    'ffn_bwd': 'ffn_bwd_kernel (FFN backward with recompute: dh, u, dx; row-block fused)',
    'ffn_ln_fwd_split': 'ffn3_fwd_kernel (csrc/ffn3.hip: w_1 + GLU + w_2 on 128-row workgroups sharing the weights through an LDS-DMA ring, hidden units split 4 ways, partial sums exchanged in the launch, bias + dropout + residual + LayerNorm; saves (value, sigmoid) tiles + u for backward)',
    'ffn_bwd_split': 'ffn3_bwd_kernel (csrc/ffn3.hip: du = dy . w_2, GLU backward on the saved tiles, dx = skip + dh . w_1, dh for the weight gradient; same structure)',
    'ffn_fwd_slab': 'ffn3_fwd_kernel<SLAB> (csrc/ffn3.hip: w_1 + GLU + w_2 on 128-row workgroups sharing the weights through an LDS-DMA ring, hidden units split 4 ways; the four slices leave 16-bit partial slabs, the next q|k|v projection finishes bias + dropout + residual + LayerNorm in its prologue; saves (value, sigmoid) tiles + u for backward)',
    'ffn_bwd_slab': 'ffn3_bwd_kernel<SLAB> (csrc/ffn3.hip: du = dy . w_2, GLU backward on the saved tiles, dh for the weight gradient, the slices\' shares of dh . w_1 as 16-bit slabs summed by the attention sub-layer\'s backward launch)',
    'rb_linear_ln': 'rb_linear_ln_kernel (csrc/rowblock.hip: the q|k|v projection with the previous FFN sub-layer\'s bias + dropout + residual + LayerNorm finished in its prologue from the four slabs)',
    'rb_linear_ln_bwd': 'rb_linear_ln_bwd_kernel (input gradient of the q|k|v projection + skip + the LayerNorm backward of the FFN sub-layer below in its epilogue)',
    'self_attention_fwd': 'attn_fwd_kernel (csrc/attention.hip: streaming-softmax attention, 128 queries per workgroup)',
    'self_attention_bwd': 'encattn_bwd_kernel (csrc/encattn.hip: one (utterance, head) staged whole in LDS, one workgroup per orientation; flops = the 5 products of the backward pass, 7 are run)',
    'dec_self_fwd': 'dec_self_fwd_kernel (csrc/declayer.hip: previous LayerNorm + q|k|v of one head + causal self-attention + its share of the output projection; grid (utterance groups, heads))',
    'dec_cross_fwd': 'dec_cross_fwd_kernel (LayerNorm + q of one head + cross-attention over the utterance memory + its share of the output projection)',
    'dec_ffn_fwd': 'dec_ffn_fwd_kernel (LayerNorm + w_1 + GLU + w_2 on 1/8 of the hidden units; grid (32-row blocks, slices))',
    'dec_ffn_bwd': 'dec_ffn_bwd_kernel (LayerNorm backward + FFN backward on the saved hidden tiles, 1/8 of the hidden units)',
    'dec_cross_bwd': 'dec_cross_bwd_kernel (LayerNorm backward + d context + cross-attention backward of one head (dq; dk, dv) + its share of dq . W_q)',
    'dec_self_bwd': 'dec_self_bwd_kernel (LayerNorm backward + d context + causal self-attention backward of one head + its share of dqkv . W_qkv)',
}


PMC_KERNEL = {'linear_wgrad_grouped': 'wgrad256_kernel', 'proj_ln_fwd': 'proj_ln_fwd_kernel', 'ln_bwd_proj': 'ln_bwd_proj_kernel',
              'ffn_ln_fwd': 'ffn_ln_fwd_kernel', 'ffn_bwd': 'ffn_bwd_kernel', 'ffn_ln_fwd_split': 'ffn3_fwd_kernel',
              'ffn_bwd_split': 'ffn3_bwd_kernel', 'ffn_fwd_slab': 'ffn3_fwd_kernel', 'ffn_bwd_slab': 'ffn3_bwd_kernel',
              'rb_linear_ln': 'rb_linear_ln_kernel', 'rb_linear_ln_bwd': 'rb_linear_ln_bwd_kernel', 'self_attention_fwd': 'attn_fwd_kernel',
              'self_attention_bwd': 'encattn_bwd_kernel', 'rb_linear': 'rb_linear_kernel', 'dec_self_fwd': 'dec_self_fwd_kernel',
              'dec_cross_fwd': 'dec_cross_fwd_kernel', 'dec_ffn_fwd': 'dec_ffn_fwd_kernel', 'dec_ffn_bwd': 'dec_ffn_bwd_kernel',
              'dec_cross_bwd': 'dec_cross_bwd_kernel', 'dec_self_bwd': 'dec_self_bwd_kernel'}


def replay_call(ops, calls, n=10):
    """launch duration of one kernel: ALL its launches of the instrumented step (each on its own operands -- in the step no layer
    finds its weights in a cache, a loop on one operand set flatters or penalises a kernel depending on what it shares through the
    L2) re-issued back to back inside ONE hipGraph, at least n launches, events on the launch stream"""
    calls = [c for c in (calls or []) if c is not None][:16]
    if not calls:
        return None
    reps = max(1, (n + len(calls) - 1) // len(calls))
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for c in calls:
                c()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            for _ in range(reps):
                for c in calls:
                    c()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (reps * len(calls))
    except Exception:                                          # noqa: BLE001
        return None


def decode_task(args):
    """BASELINE configs[4] (C5) through tools/decode_bench.py: one JSON line with the same contract keys"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('decode_bench', os.path.join(ROOT, 'tools', 'decode_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = ['--mode', args.mode, '--iters', str(args.steps), '--warmup', str(args.warmup)]
    if args.no_cpu_baseline or not args.full:
        argv.append('--no-cpu-baseline')
    outputs = {} if args.dump_outputs else None
    mod.main(argv, outputs=outputs)
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)


def main():
    args = parse()
    if args.task == 'decode':
        assert args.gpus == 1, 'the decode task runs on one GPU (utterances are independent: replicas only)'
        return decode_task(args)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        relaunch_under_torchrun(args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    assert torch.cuda.is_available(), 'bench.py needs a GPU (the product has no CPU path)'
    # OTR_BENCH_ONE_GPU=1 (tests on a one-GPU box only): every rank on cuda:0, collectives over gloo -- exercises the N > 1 control
    # flow (staged step, collectives between the graphs, breakdown passes) end to end; the numbers mean nothing
    one_gpu = os.environ.get('OTR_BENCH_ONE_GPU') == '1'
    if one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        if one_gpu:
            dist.init_process_group('gloo', init_method='env://')
        else:
            dist.init_process_group('nccl', init_method='env://', device_id=dev)

    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam

    cfg = syn.c2_model(residual_dropout=args.dropout) if args.model == 'transformer' else syn.conformer_model(False, args.dropout)
    inputs, targets = syn.synthetic_batch(args.batch, args.frames, 80, 4234, 15, seed=rank)
    inputs = {k: v.to(dev) for k, v in inputs.items()}
    targets = {k: v.to(dev) for k, v in targets.items()}

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def build(mode, overlap=False, payload=None):
        """model + replica engine + optimizer + (captured) step of the workload in compute mode `mode`; overlap: the staged
        two-collective step; payload: None = the fp32 gradient buffer travels, torch.bfloat16 = a 16-bit copy of it"""
        ops.set_compute_dtype(mode)
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 1234)           # identical replicas on every rank
        model = model.to(dev).train()
        ops.set_stage_split(overlap)
        dp = FlatDataParallel(model, early_modules=([model.decoder] + ([model.assistor] if hasattr(model, 'assistor') else [])) if overlap else None,
                              grad_comm_dtype=payload)
        dp.broadcast_parameters()
        opt = FusedAdam(dp, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-6, clip_grad=5.0,
                        noam=dict(model_size=cfg['encoder']['d_model'], warmup_steps=12000, factor=1.0))   # *_baseline.yaml train section
        class _LossRef:
            """the loss of the last step: the tensor the step itself wrote (under a hipGraph that is static memory of the graph's
            pool, rewritten by every replay), so reading it out costs no copy launch inside the step"""
            t = torch.zeros((), device=dev)

            def item(self):
                return self.t.item()
        loss_buf = _LossRef()

        stages = []
        # N = 1: nothing sits between the backward pass and the optimizer, so the WHOLE step is one hipGraph (--opt-in-graph off: the
        # optimizer's launches follow the replay eagerly, as they must at N > 1 where the all-reduce sits in between)
        whole = world == 1 and not overlap and args.opt_in_graph == 'on' and not args.no_graph

        def stage1():
            dp.zero_grad(next_dropout_step=True)   # the gradient fill and the dropout seed's step in one launch
            loss, _ = dp(inputs, targets)
            ops.backward(loss)                    # staged: stops at the encoder / decoder cut (ops.early_mark); else the whole pass
            loss_buf.t = loss.detach()
            stages[:] = ops.take_stages()

        def stage2():
            for x, leaf in reversed(stages):
                x.backward(leaf.grad)

        def fwd_bwd():
            ops.set_stage_split(overlap)          # process-wide switch, read by the forward pass: several runs may be alive
            stage1()
            if overlap:
                dp.start_early_reduce()
                stage2()

        graph, graph2 = None, None
        if not args.no_graph:
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        fwd_bwd()
                        if overlap:
                            dp.all_reduce_gradients()     # consumes the early collective of the warm-up passes
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                # N > 1: the process group's watchdog thread polls its events while this thread captures; only THIS thread's calls
                # are policed then (the default, global, mode lets a foreign thread's call invalidate the capture)
                cap = {'capture_error_mode': 'thread_local'} if world > 1 else {}
                graph = torch.cuda.CUDAGraph()
                with ops.graph_capture(graph, **cap):
                    stage1()
                    if whole:
                        opt.step(1.0)
                if overlap:
                    graph2 = torch.cuda.CUDAGraph()
                    with ops.graph_capture(graph2, pool=graph.pool(), **cap):
                        stage2()
            except Exception as e:                                # noqa: BLE001
                if rank == 0:
                    print('hipGraph capture failed (%s: %s); running eagerly' % (type(e).__name__, e), file=sys.stderr)
                graph, graph2 = None, None
                torch.cuda.synchronize()

        def run_fwd_bwd():
            if graph is None:
                fwd_bwd()
                return
            graph.replay()
            if overlap:
                # (a second graph launch costs ~0.2 ms on this stack -- measured at N = 1 with forward / backward as two graphs and
                # with this staged step: 4.40 -> 4.62 ms, the host calls take 0.05 + 0.18 ms and never block -- which the early
                # group's 37 % of the all-reduce has to buy back: break-even near 0.55 ms of all-reduce time)
                dp.start_early_reduce()                   # eager, on the side stream: beside the second graph
                graph2.replay()

        def step():
            run_fwd_bwd()
            if whole and graph is not None:
                return
            scale, _ = dp.all_reduce_gradients()
            opt.step(scale)
        return dict(whole=whole, dp=dp, opt=opt, fwd_bwd=fwd_bwd, run_fwd_bwd=run_fwd_bwd, step=step, graph=graph, loss_buf=loss_buf, overlap=overlap)

    def timed(step, warmup, steps):
        """W untimed steps, then EXACTLY K steps bracketed by barrier + synchronize on both sides; max over ranks"""
        for _ in range(warmup):
            step()
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        fence()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    # N > 1: which form of the step?  `off` = the single collective north_star states; `on` = the staged two-collective step; `auto` =
    # both are built and MEASURED here (a few untimed steps each, max over ranks, so every rank takes the same decision) and the
    # contract region runs on the faster one.  N = 1: no collective, one graph.
    forms = None
    if world > 1 and args.overlap == 'auto':
        cands = {'single_collective': build(args.mode, overlap=False), 'staged_two_collectives': build(args.mode, overlap=True)}
        forms = {k: timed(r['step'], 3, args.calib_steps) / args.calib_steps * 1e3 for k, r in cands.items()}
        chosen = min(forms, key=lambda k: forms[k])
        run = cands.pop(chosen)
        cands.clear()
        torch.cuda.empty_cache()
        forms = {'ms_per_step_calibration': forms, 'chosen': chosen, 'calib_steps': args.calib_steps,
                 'note': 'both forms of the N > 1 step measured in this invocation before the contract region (untimed, max over ranks)'}
    else:
        run = build(args.mode, overlap=(args.overlap == 'on'))      # N = 1 / explicit choice; --overlap on at N = 1 is the A/B of DESIGN.md section 7
    ops.set_stage_split(run['overlap'])
    dp, opt, fwd_bwd, step, graph, loss_buf = (run[k] for k in ('dp', 'opt', 'fwd_bwd', 'step', 'graph', 'loss_buf'))
    run_fwd_bwd = run['run_fwd_bwd']

    used_graph = graph is not None
    elapsed = timed(step, args.warmup, args.steps)

    # ---- --full, untimed: where the step time goes (every rank: the collectives must match)
    final_loss, final_stats = float(loss_buf.item()), opt.stats()      # state at the end of the timed region
    if args.dump_outputs and rank == 0:       # before the extras below run more steps on the same replica
        dump_outputs(args.dump_outputs, train_step_outputs(run, final_loss))
    extras = args.full and not args.no_extras
    parts = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    windows = None
    if extras:
        # box-to-box and run-to-run spread is ~1.5 %: besides the contract's K steps (`value`), five more windows of K steps each,
        # timed the same way (barrier + synchronize on both sides, max over ranks); their median is the robust figure
        windows = [timed(step, 0, args.steps) / args.steps * 1e3 for _ in range(5)]
        final_loss, final_stats = float(loss_buf.item()), opt.stats()
    if extras:
        acc = [0.0, 0.0]
        for _ in range(5):
            ev[0].record()
            run_fwd_bwd()
            ev[1].record()
            if not (run['whole'] and graph is not None):
                scale, _ = dp.all_reduce_gradients()
                opt.step(scale)
            ev[2].record()
            torch.cuda.synchronize()
            acc[0] += ev[0].elapsed_time(ev[1])
            acc[1] += ev[1].elapsed_time(ev[2])
        parts = {'fwd_bwd_ms': acc[0] / 5, 'allreduce_optimizer_ms': acc[1] / 5}
        if run['whole'] and graph is not None:
            parts = {'whole_step_graph_ms': acc[0] / 5,
                     'note': 'N = 1: forward, backward and the optimizer launches are ONE hipGraph (--opt-in-graph off separates them)'}
    if world > 1 and extras:     # the collective on its own: 5 all-reduces of the flat gradient buffer, events on the stream
        ev[0].record()
        for _ in range(5):
            dp.all_reduce_gradients()
        ev[1].record()
        torch.cuda.synchronize()
        parts['allreduce_ms'] = ev[0].elapsed_time(ev[1]) / 5
        # what the step pays for it: the same steps with every collective skipped (gradients are then wrong: timing only)
        dp.skip_collectives = True
        t_skip = timed(step, 2, args.steps) / args.steps * 1e3
        dp.skip_collectives = False
        parts['ms_per_step_without_collectives'] = t_skip
        parts['exposed_allreduce_ms'] = elapsed / args.steps * 1e3 - t_skip
        parts['overlap'] = bool(run['overlap'])
        parts['form'] = 'staged_two_collectives' if run['overlap'] else 'single_collective'
        parts['forms_measured'] = forms
        parts['allreduce_bytes'] = dp.flat_grad.numel() * dp.flat_grad.element_size()
        parts['nranks'] = dist.get_world_size()
        parts['backend'] = dist.get_backend()
        # the same step with a bf16 gradient payload (half the xGMI bytes; the sum is rounded to bf16: NOT the parity mode, reported
        # beside the contract value, never as it)
        try:
            run_p = build(args.mode, overlap=run['overlap'], payload=torch.bfloat16)
            t_p = timed(run_p['step'], 3, args.steps) / args.steps * 1e3
            parts['bf16_payload'] = {'ms_per_step': t_p, 'value': args.batch * world / (t_p * 1e-3), 'allreduce_bytes': dp.flat_grad.numel() * 2,
                                     'skipped': run_p['opt'].stats()['skipped']}
            del run_p
            torch.cuda.empty_cache()
        except Exception as e:                                     # noqa: BLE001  (every rank fails alike: same code, same sizes)
            parts['bf16_payload'] = {'error': '%s: %s' % (type(e).__name__, e)}
        ops.set_stage_split(run['overlap'])
        ops.set_compute_dtype(args.mode)
    kern = None
    if rank == 0 and extras:
        dp.skip_collectives = True            # rank 0 alone runs this pass: it must not start a collective (staged step: the early group's)
        try:
            kern = instrumented_step(ops, fwd_bwd, args.mode)
        finally:
            dp.skip_collectives = False
    if world > 1:
        dist.barrier()

    out = None
    if rank == 0:
        global_batch = args.batch * world
        utt_s = global_batch * args.steps / elapsed
        flops_utt = syn.flops_per_utt(cfg, args.frames, 15) if args.model == 'transformer' else 63207.57e6
        peak = PEAK_F32_TFLOPS if args.mode == 'fp32' else PEAK_16BIT_TFLOPS
        out = {
            'metric': 'utterances/sec (80-d fbank, ~1000 frames) train fwd+bwd', 'value': utt_s,
            'unit': 'utterances/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': elapsed / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': args.mode, 'data': 'synthetic',
            'config': {'workload': 'AISHELL-1 transformer_baseline.yaml (+input_size 80), 12 enc / 6 dec layers, '
                                   'B=%d/GPU x %d frames x 80-d fbank, 15 decoder rows, V=4234, residual_dropout %s; '
                                   'step = fwd + bwd + grad all-reduce + clip/Adam/Noam' % (args.batch, args.frames, args.dropout),
                       'global_batch': global_batch, 'frames': args.frames, 'parallelism': 'dp%d' % world,
                       'hipgraph': used_graph},
            'loss': final_loss, 'optimizer': final_stats,
            'model_tflops_per_s': utt_s * flops_utt / 1e12,
            'model_mfma_frac': utt_s * flops_utt / 1e12 / world / peak,
        }
        st = final_stats
        if st.get('faults', 0) != 0:
            out['INVALID'] = ('%d bounded inter-workgroup waits gave up (wrong gradient sums possible): %d optimizer updates were '
                              'skipped' % (int(st['faults']), int(st['skipped'])))
        elif st['skipped'] != 0 or not (st['grad_sqnorm'] == st['grad_sqnorm'] and st['grad_sqnorm'] < float('inf')):
            out['INVALID'] = 'non-finite gradient norm: %d optimizer updates were skipped' % int(st['skipped'])
        if parts:
            out['step_breakdown'] = parts
        if windows:
            ws_ = sorted(windows)
            out['windows'] = {'ms_per_step': windows, 'median_ms_per_step': ws_[len(ws_) // 2],
                              'median_value': global_batch / (ws_[len(ws_) // 2] * 1e-3), 'steps_per_window': args.steps,
                              'note': 'five further windows of K steps, timed like the contract region; `value` is the contract region'}
        if kern:
            # HBM bytes per launch and MFMA-busy cycles from separate rocprofv3 --pmc passes of this command (tools/gpu_pmc_step.sh
            # -> profiles/r03_pmc_step.json; regenerate whenever a kernel changes: the record carries the commit it was taken at)
            pmc_db, pmc_file = {}, None
            for cand_file in ('r06_pmc_step.json', 'r05_pmc_step.json', 'r04_pmc_step.json', 'r03_pmc_step.json'):
                try:
                    pmc_db = json.load(open(os.path.join(ROOT, 'profiles', cand_file)))
                    pmc_file = os.path.join('profiles', cand_file)
                    break
                except Exception:                                          # noqa: BLE001
                    continue

            def pmc_of(name):
                # records are keyed by kernel, grid size AND duration class (tools/pmc_summary.py): a kernel launched on several
                # problem sizes (wgrad256_kernel: the M = B x T' group and the decoder's group share one persistent grid) has one
                # record each; the line of the step's dominant launch of that kernel is the one with the largest share of time
                pat = PMC_KERNEL.get(name.split(' ')[0])
                hits = [v for k, v in pmc_db.items() if pat and pat in k and isinstance(v, dict) and not k.startswith('_')]
                return max(hits, key=lambda v: v.get('share_of_kernel_time', 0.0)) if hits else {}
            # in-step durations of the same kernels from the committed rocprofv3 trace of the replayed step (tools/graph_gaps.py):
            # printed beside the live timings, not instead of them
            step_db = {}
            for cand_file in ('r06_step_kernels.json', 'r05_step_kernels.json'):
                try:
                    step_db = json.load(open(os.path.join(ROOT, 'profiles', cand_file)))
                    break
                except Exception:                                      # noqa: BLE001
                    continue

            def in_step_us(name):
                pat = PMC_KERNEL.get(name.split(' ')[0])
                hits = [v for k, v in step_db.items() if pat and k.startswith(pat) and isinstance(v, dict) and not k.startswith('_')]
                if not hits:
                    return None
                h = max(hits, key=lambda v: v['avg_us'] * v['launches_per_step'])
                return h['max_us'] if name == 'linear_wgrad_grouped' else h['avg_us']    # the M = B x T' launch is the longest of its name
            lines = {}
            for name, a in kern.items():
                if a['flops_per_launch'] <= 0:
                    continue
                pm = pmc_of(name)
                lines[name] = {'bound': 'mfma', 'kernel': KERNEL_LABEL.get(name, name), 'achieved': a['achieved'], 'peak': peak,
                               'unit': 'TFLOP/s', 'frac': a['frac'],
                               'traffic': pm.get('hbm_bytes_per_launch'),
                               'algorithmic_bytes': a['algorithmic_bytes_per_launch'] or None,
                               'mfma_busy_frac_pmc': pm.get('mfma_busy_frac'),
                               'avg_launch_ms': a['avg_launch_ms'], 'launches_per_step': a['launches'],
                               'ms_per_step': a['total_ms'], 'timed': 'events around every launch inside one eager training step',
                               'avg_launch_us_in_step_rocprof': in_step_us(name)}
            if lines:
                # EVERY line is re-timed before it is graded (no duration from the eager brackets, which also hold the
                # host's launch gap): the launches of that kernel in the step, each on its own operands, re-issued back to back inside
                # one hipGraph with events on the launch stream.  A kernel whose launches cannot be re-issued is dropped from the
                # table (named in `roofline_untimed`), not graded on the bracket.
                untimed = []
                for name in list(lines):
                    d = lines[name]
                    if name == 'linear_wgrad_grouped':
                        rep = replay_dominant(ops, name, args.mode)
                        if rep:           # 199 flop per algorithmic byte < the 312 flop/B ridge: this launch is HBM-bound
                            d.update(avg_launch_ms_eager_bracket=d['avg_launch_ms'], avg_launch_ms=rep['ms'], bound='hbm',
                                     algorithmic_bytes=rep['bytes'], achieved=rep['bytes'] / (rep['ms'] * 1e-3) / 1e9,
                                     peak=PEAK_HBM_GBS, unit='GB/s', tflops=rep['flops'] / (rep['ms'] * 1e-3) / 1e12,
                                     problems=rep['problems'], rows=rep['rows'])
                            d['frac'] = d['achieved'] / PEAK_HBM_GBS
                            d['mfma_frac'] = d['tflops'] / peak
                            d['ms_per_step'] = rep['ms']
                            d['launches_per_step'] = 1
                            d['timed'] = ('10 back-to-back launches of the longest-contraction group (M = B x T\') on the operands of the step '
                                          'inside one hipGraph, events on the launch stream; the short-contraction launches of this name are '
                                          'not part of this line')
                        else:
                            untimed.append(name)
                            del lines[name]
                    else:
                        ms = replay_call(ops, kern[name].get('calls'))
                        if ms:
                            d.update(avg_launch_ms_eager_bracket=d['avg_launch_ms'], avg_launch_ms=ms,
                                     achieved=kern[name]['flops_per_launch'] / (ms * 1e-3) / 1e12)
                            d['frac'] = d['achieved'] / peak
                            d['ms_per_step'] = ms * d['launches_per_step']
                            d['timed'] = ('the launches of this kernel in the step, each on its own operands, re-issued back to back (>= 10) '
                                          'inside one hipGraph, events on the launch stream')
                        else:
                            untimed.append(name)
                            del lines[name]
                if untimed:
                    out['roofline_untimed'] = untimed
                # the table must fit inside the step it claims to describe
                step_ms = elapsed / args.steps * 1e3
                sum_ms = sum(v['ms_per_step'] for v in lines.values())
                out['roofline_sum_check'] = {'sum_ms_per_step': sum_ms, 'step_ms': step_ms, 'ok': bool(sum_ms <= step_ms),
                                             'note': 'sum of ms_per_step over every graded kernel (graph-replay durations) against the timed step'}
                if sum_ms > step_ms and rank == 0:
                    print('bench.py: roofline table sums to %.3f ms > step %.3f ms' % (sum_ms, step_ms), file=sys.stderr)
                # The FFN sub-layer is graded against the bound SURVEY.md 8(d) names for it: MFMA (frac = flops / launch duration /
                # 2.5 PFLOP/s).  Its MINIMAL I/O (x, x16, y, y16, z, the packed weights once: what a recomputing backward would
                # need) puts it at ~700 flop/B, far above the 312 flop/B ridge; the tiles it saves for the backward pass are a
                # choice of this implementation, not algorithmic traffic.  The HBM view is kept as a secondary key.
                for name in ('ffn_fwd_slab', 'ffn_bwd_slab', 'ffn_ln_fwd_split', 'ffn_bwd_split', 'ffn_ln_fwd', 'ffn_bwd'):
                    if name in lines and lines[name].get('algorithmic_bytes'):
                        d = lines[name]
                        M_, F_, d_ = args.batch * ((((args.frames - 3) // 2 + 1) - 3) // 2 + 1), cfg['encoder']['d_ff'], cfg['encoder']['d_model']
                        min_io = M_ * d_ * (4 + 2 + 4 + 2 + 4) + 6 * F_ * d_ if 'fwd' in name else M_ * d_ * (2 + 4 + 4) + 6 * F_ * d_
                        d['hbm_view'] = {'algorithmic_bytes_minimal_io': min_io, 'bytes_incl_saved_tiles': d['algorithmic_bytes'],
                                         'achieved_GBs_minimal_io': min_io / (d['avg_launch_ms'] * 1e-3) / 1e9,
                                         'achieved_GBs_incl_saved_tiles': d['algorithmic_bytes'] / (d['avg_launch_ms'] * 1e-3) / 1e9,
                                         'frac_of_hbm_peak_incl_saved_tiles': d['algorithmic_bytes'] / (d['avg_launch_ms'] * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                         'flop_per_byte_minimal_io': kern[name]['flops_per_launch'] / min_io}
                        d['algorithmic_bytes'] = min_io
                dom = max(lines, key=lambda k: lines[k]['ms_per_step'])     # launches x duration, every kernel a candidate
                d = lines.pop(dom)
                d['flops_per_launch'] = kern[dom]['flops_per_launch']
                d['share_of_step'] = d['ms_per_step'] / (elapsed / args.steps * 1e3)
                d['pmc_source'] = '%s (%s)' % (pmc_file, pmc_db.get('_meta', {}).get('commit', 'absent')) if pmc_db else None
                out['roofline'] = d
                keep = sorted(lines, key=lambda k: -lines[k]['ms_per_step'])[:24]
                out['roofline_kernels'] = {k: lines[k] for k in keep}
    # ---- BASELINE.json configs[1] names bf16: the same workload, steps and timing in bf16 mode (8 mantissa bits: logits
    #      4e-3 from the fp32 reference, outside the north star's 1e-3 -- why the headline value is the fp16 line).  Every rank
    #      takes part (the step holds the collective); after the replays above, which need the primary mode's operands
    bf16_line = None
    if args.mode != 'bf16' and args.model == 'transformer' and extras and not args.no_bf16_line:
        overlap_primary = run['overlap']
        del run, dp, opt, fwd_bwd, run_fwd_bwd, step, graph, kern    # free the primary replica (graph pool, 2.2 GB of saved activations)
        torch.cuda.empty_cache()
        run2 = build('bf16', overlap=overlap_primary)
        el2 = timed(run2['step'], args.warmup, args.steps)
        st2 = run2['opt'].stats()
        bf16_line = {'value': args.batch * world * args.steps / el2, 'unit': 'utterances/s', 'ms_per_step': el2 / args.steps * 1e3,
                     'steps': args.steps, 'warmup': args.warmup, 'loss': float(run2['loss_buf'].item()), 'skipped': st2['skipped'],
                     'hipgraph': run2['graph'] is not None}
        hipgraph = run2['graph'] is not None
        del run2
        ops.set_compute_dtype(args.mode)
    if rank == 0:
        if bf16_line is not None:
            for mode_, slot in (('bf16', bf16_line), (args.mode, out)):
                for rnd in ('r06', 'r05', 'r04', 'r03'):      # the measured parity of that mode at this batch (tests/test_gpu_headline.py -> profiles/)
                    try:
                        pr = json.load(open(os.path.join(ROOT, 'profiles', '%s_parity_headline_%s.json' % (rnd, mode_))))
                    except Exception:                                          # noqa: BLE001
                        continue
                    slot['logits_rel_vs_oracle'] = pr.get('logits_rel')
                    slot['loss_rel_vs_oracle'] = pr.get('loss_rel')
                    # the north star's bar: logits and loss within 1e-3 relative of the reference
                    slot['parity_bar_met'] = bool(pr.get('logits_rel') is not None and pr['logits_rel'] < 1e-3
                                                  and (pr.get('loss_rel') is None or pr['loss_rel'] < 1e-3))
                    slot['parity_source'] = 'profiles/%s_parity_headline_%s.json' % (rnd, mode_)
                    break
            out['bf16'] = bf16_line
        if args.model != 'transformer':
            out['config']['workload'] = out['config']['workload'].replace('transformer_baseline.yaml (+input_size 80), 12 enc / 6 dec layers', 'conformer_baseline.yaml, 12 conformer blocks / 6 dec layers')
        if world == 1 and args.full and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(args)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
