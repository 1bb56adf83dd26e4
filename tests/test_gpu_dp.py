"""GPU (-m gpu): the N > 1 data-parallel path with the REAL HIP model.

gpurun boxes have one GPU, so two processes share cuda:0 and all-reduce over gloo (which moves CUDA tensors through the
host): everything above the collective -- utterance sharding, in-place flat gradients, deferred grouped weight
gradients, 1/N folded into the fused optimizer, the 16-bit weight shadows following broadcast_parameters -- is the code
the 8-GPU RCCL run uses.  The reduced gradient is checked against the oracle's mean-of-shard-losses gradient
(nn.DataParallel semantics, train/trainer.py:208).  The library-owned RCCL communicator
(otr_allreduce_*) is exercised at world size 1."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from opentransformer_amd import synthetic as syn
from tests import helpers as H

pytestmark = pytest.mark.gpu
BATCH = dict(batch=4, frames=200, feat_dim=80, vocab=100, tgt_len=10, seed=0, lengths=[200, 180, 150, 97], tgt_lengths=[10, 8, 10, 5])


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, mode, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    torch.cuda.set_device(0)
    ops.set_compute_dtype(mode)
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 77 + 5 * rank)          # replicas start DIFFERENT: broadcast must fix weights AND shadows
    model = model.to('cuda').train()
    dp = FlatDataParallel(model)
    dp.broadcast_parameters(0)
    opt = FusedAdam(dp, lr=1e-3, loss_scale=(1024.0 if mode == 'fp16' else None))
    inputs, targets = syn.synthetic_batch(**BATCH)
    sh = slice(rank * 2, rank * 2 + 2)                                 # contiguous utterance shards
    dp.zero_grad()
    loss, _ = dp({k: v[sh].cuda() for k, v in inputs.items()}, {k: v[sh].cuda() for k, v in targets.items()})
    loss.backward()
    scale, _ = dp.all_reduce_gradients()
    ls = float(opt.state[6]) or 1.0
    grads = {k: (p.grad.detach().float() * (scale / ls)).cpu() for k, p in model.named_parameters()}
    before = dp.flat_param.clone()
    opt.step(scale)
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({'grads': grads, 'loss': loss.item(), 'stats': opt.stats(), 'moved': float((dp.flat_param - before).abs().max()),
                    'shadow_ok': bool(torch.equal(dp.flat_param_lp.float(), dp.flat_param.to(dp.flat_param_lp.dtype).float()))
                    if dp.flat_param_lp is not None else True}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_two_ranks_one_gpu_real_model_matches_oracle(tmp_path, mode):
    from oracle import otrans_oracle as orc
    out = str(tmp_path / 'r0.pt')
    mp.spawn(_worker, args=(2, _free_port(), mode, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    inputs, targets = syn.synthetic_batch(**BATCH)
    parts = H.require_grad(H.filled_state(cfg, seed=77))               # rank 0's weights (broadcast source)
    losses = []
    for r in range(2):
        sh = slice(r * 2, r * 2 + 2)
        l, _ = orc.speech2text_forward(parts, cfg, {k: v[sh] for k, v in inputs.items()}, {k: v[sh] for k, v in targets.items()})
        losses.append(l)
    (0.5 * (losses[0] + losses[1])).backward()                          # mean of per-shard losses = DataParallel semantics
    flat = H.flat_named(parts)
    assert abs(got['loss'] - losses[0].item()) < (1e-4 if mode == 'fp32' else 1e-3) * abs(losses[0].item())
    worst = 0.0
    for k, g in got['grads'].items():
        ref = flat[k].grad
        worst = max(worst, float((g - ref).norm() / max(float(ref.norm()), 1e-3)))
    assert worst < (5e-4 if mode == 'fp32' else 3e-2), worst          # measured 1.6e-2 in fp16 (a near-zero bias gradient)
    assert got['stats']['skipped'] == 0 and got['moved'] > 0 and got['shadow_ok']


def _fault_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    torch.cuda.set_device(0)
    ops.set_compute_dtype('fp16')
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    model = ota.SpeechToText(cfg)
    syn.fill_state_dict_(model.state_dict(), 77)
    model = model.to('cuda').train()
    dp = FlatDataParallel(model, grad_comm_dtype=(torch.bfloat16 if rank >= 0 and os.environ.get('OTR_TEST_PAYLOAD') == 'bf16' else None))
    dp.broadcast_parameters(0)
    opt = FusedAdam(dp, lr=1e-3, loss_scale=1024.0)
    inputs, targets = syn.synthetic_batch(**BATCH)
    sh = slice(rank * 2, rank * 2 + 2)
    res = []
    for step in range(2):
        dp.zero_grad()
        loss, _ = dp({k: v[sh].cuda() for k, v in inputs.items()}, {k: v[sh].cuda() for k, v in targets.items()})
        loss.backward()
        if step == 0 and rank == 1:
            ops.fault_counter(torch.device('cuda', 0)).add_(3)     # rank 1 only: a bounded wait of its backward pass gave up
        before = dp.flat_param.clone()
        scale, _ = dp.all_reduce_gradients()
        opt.step(scale)
        torch.cuda.synchronize()
        res.append({'moved': float((dp.flat_param - before).abs().max()), 'stats': opt.stats(),
                    'word': int(ops.fault_counter(torch.device('cuda', 0)).item())})
    torch.save({'res': res, 'param': dp.flat_param.cpu()}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('payload', ['fp32', 'bf16'])
def test_fault_on_one_rank_skips_the_update_on_every_rank(tmp_path, payload, monkeypatch):
    """ADVICE r03 (dp.py:276): the sticky fault word is local to a rank, but the gradient it taints is summed into every replica.
    It now rides through the same collective: BOTH ranks skip the update of that step (parameters unchanged, same counters) and
    apply the next one -- the replicas stay identical."""
    monkeypatch.setenv('OTR_TEST_PAYLOAD', payload)
    out = str(tmp_path / 'r%d.pt')
    mp.spawn(_fault_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0, weights_only=False), torch.load(out % 1, weights_only=False)
    for r in (r0, r1):
        first, second = r['res']
        assert first['moved'] == 0.0 and first['stats']['skipped'] == 1 and first['stats']['faults'] == 3 and first['word'] == 0
        assert second['moved'] > 0 and second['stats']['skipped'] == 1 and second['stats']['step'] == 1
    assert torch.equal(r0['param'], r1['param'])


def _split_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel
    torch.cuda.set_device(0)
    ops.set_compute_dtype('fp16')
    cfg = syn.c1_model(0.0, ctc_weight=0.3)
    inputs, targets = syn.synthetic_batch(**BATCH)
    sh = slice(rank * 2, rank * 2 + 2)
    res = {}
    ins, tgs = {k: v[sh].cuda() for k, v in inputs.items()}, {k: v[sh].cuda() for k, v in targets.items()}
    for name in ('single', 'split', 'staged', 'staged_graphs'):
        model = ota.SpeechToText(cfg)
        syn.fill_state_dict_(model.state_dict(), 77)
        model = model.to('cuda').train()
        dp = FlatDataParallel(model, early_modules=[model.decoder, model.assistor] if name != 'single' else None)
        ops.set_stage_split(name.startswith('staged'))
        try:
            if name == 'staged_graphs':
                # bench.py's N > 1 step: stage 1 and stage 2 as two hipGraphs, the early collective issued between their replays
                stages = []

                def stage1():
                    dp.zero_grad()
                    loss, _ = dp(ins, tgs)
                    loss.backward()
                    stages[:] = ops.take_stages()

                def stage2():
                    for x, leaf in reversed(stages):
                        x.backward(leaf.grad)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        stage1(); dp.start_early_reduce(); stage2(); dp.all_reduce_gradients()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with ops.graph_capture(g1, capture_error_mode='thread_local'):        # as bench.py captures at N > 1
                    stage1()
                with ops.graph_capture(g2, pool=g1.pool(), capture_error_mode='thread_local'):
                    stage2()
                for _ in range(2):                      # replayed twice: nothing of a replay may leak into the next
                    g1.replay()
                    dp.start_early_reduce()
                    res[name + '_issued'] = dp._early_state is not None
                    g2.replay()
                    scale, _ = dp.all_reduce_gradients()
            else:
                dp.zero_grad()
                loss, _ = dp(ins, tgs)
                if name == 'staged':
                    n_st = len(dp.backward_staged(loss))
                    assert n_st == 1
                    res[name + '_issued'] = True
                else:
                    loss.backward()
                    res[name + '_issued'] = dp._early_state is not None
                scale, _ = dp.all_reduce_gradients()
            torch.cuda.synchronize()
            res[name] = {k: (p.grad.detach().float() * scale).cpu() for k, p in model.named_parameters()}
            res[name + '_early'] = dp.early_end
        finally:
            ops.set_early_callback(None)
            ops.set_stage_split(False)
    if rank == 0:
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_group_allreduce_with_the_real_model(tmp_path):
    """decoder + CTC head reduced on a side stream as soon as their backward is done (ops.early_mark on the
    encoder output fires inside the pass, after their deferred weight-gradient launches), the rest at the end: the same reduced
    gradient as the single collective.  Two ranks on one GPU over gloo."""
    out = str(tmp_path / 'r0.pt')
    mp.spawn(_split_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    assert got['split_issued'] and not got['single_issued'] and got['split_early'] > 0 and got['single_early'] == 0
    assert got['staged_issued'] and got['staged_graphs_issued']
    # 'staged': the graph-cut backward of ops.set_stage_split (loss.backward() stops at the encoder output, the early group's
    # collective starts, the encoder's backward follows); 'staged_graphs': the same as two replayed hipGraphs (bench.py at N > 1)
    for name in ('split', 'staged', 'staged_graphs'):
        worst = 0.0
        for k, g in got[name].items():
            ref = got['single'][k]
            worst = max(worst, float((g - ref).norm() / max(float(ref.norm()), 1e-6)))
        assert worst < 1e-5, (name, worst)   # two runs of one backward pass differ in the last bits (float atomics), nothing more


def test_library_owned_rccl_communicator_world_one():
    """otr_allreduce_unique_id / init / run / destroy on a single-rank communicator: sum over one rank = identity, issued on
    the compute stream, for the fp32 buffer and for a bf16 payload"""
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel
    ops.set_compute_dtype('fp16')
    try:
        model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
        syn.fill_state_dict_(model.state_dict(), 3)
        for payload in (None, torch.bfloat16):
            dp = FlatDataParallel(model.to('cuda').train(), comm='rccl', grad_comm_dtype=payload)
            dp.flat_grad.copy_(torch.randn_like(dp.flat_grad))
            want = dp.flat_grad.clone() if payload is None else dp.flat_grad.to(payload).float()
            scale, _ = dp.all_reduce_gradients(force=True)
            torch.cuda.synchronize()
            assert scale == 1.0 and torch.equal(dp.flat_grad, want)
            dp.close()
    finally:
        ops.set_compute_dtype('bf16')


def _rccl2_worker(rank, world, port, out):
    import threading
    # RCCL's rendezvous is host-side sockets: a refusal is an error code, but a hang must not take the test run with it
    def give_up():
        torch.save({'rank': rank, 'init': 'timeout', 'uid': b'', 'uid_nonzero': False}, out % rank)
        os._exit(0)
    threading.Timer(90.0, give_up).start()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import ctypes as C
    import opentransformer_amd as ota
    from opentransformer_amd import ops, _lib
    from opentransformer_amd.dp import FlatDataParallel
    torch.cuda.set_device(0)
    ops.set_compute_dtype('fp16')
    model = ota.SpeechToText(syn.c1_model(0.0, ctc_weight=0.3))
    syn.fill_state_dict_(model.state_dict(), 3)
    dp = FlatDataParallel(model.to('cuda').train(), comm='rccl')
    res = {'rank': rank}
    # (i) the plumbing of dp._rccl_handle, step by step: rank 0's unique id reaches every rank through the torch.distributed store
    lib = _lib.load()
    uid = C.create_string_buffer(128)
    if rank == 0:
        _lib.check(lib.otr_allreduce_unique_id(uid), 'otr_allreduce_unique_id')
    box = [uid.raw]
    dist.broadcast_object_list(box, src=0)
    res['uid'] = bytes(box[0])
    res['uid_nonzero'] = any(box[0])
    # (ii) the engine's own path: init with (rank, world) = (rank, 2).  Two ranks on ONE device: RCCL may refuse ("duplicate GPU");
    # then the refusal must arrive as an error of the C ABI with a message, on both ranks, not as a hang or a crash
    try:
        dp._rccl_handle()
        res['init'] = 'ok'
    except _lib.OtransHipError as e:
        res['init'] = 'refused: %s' % e
    if res['init'] == 'ok':
        dp.flat_grad.fill_(float(rank + 1))
        scale, _ = dp.all_reduce_gradients()
        torch.cuda.synchronize()
        res['sum_ok'] = bool(scale == 0.5 and torch.equal(dp.flat_grad, torch.full_like(dp.flat_grad, 3.0)))
        dp.close()
    torch.save(res, out % rank)
    dist.barrier()
    dist.destroy_process_group()
    os._exit(0)


def test_library_owned_rccl_communicator_two_processes(tmp_path):
    """comm='rccl' across TWO processes -- otr_allreduce_unique_id on rank 0, the 128 bytes shipped through the
    gloo-bootstrapped torch.distributed group, otr_allreduce_init(rank, 2) on both.  A box with one GPU puts both ranks on one
    device, which RCCL may refuse: the test then checks that the refusal is an error of the C ABI on both ranks (and skips the sum);
    where RCCL accepts it, the in-place sum over the two ranks is checked."""
    out = str(tmp_path / 'r%d.pt')
    ctx = mp.spawn(_rccl2_worker, args=(2, _free_port(), out), nprocs=2, join=False)
    deadline = 150
    import time
    t0 = time.time()
    while not ctx.join(timeout=5):
        if time.time() - t0 > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail('RCCL rendezvous of two processes did not return')
    got = [torch.load(out % r, weights_only=False) for r in range(2)]
    if any(g['init'] == 'timeout' for g in got):
        pytest.skip('RCCL rendezvous of two ranks on one device did not return within 90 s on this box: %s' % [g['init'] for g in got])
    assert got[0]['uid'] == got[1]['uid'] and got[0]['uid_nonzero']          # the id travelled
    assert (got[0]['init'] == 'ok') == (got[1]['init'] == 'ok'), got           # both ranks see the same outcome
    if got[0]['init'] == 'ok':
        assert got[0]['sum_ok'] and got[1]['sum_ok']
    else:
        assert all('RCCL error' in g['init'] or 'allreduce' in g['init'] for g in got), got
        print('RCCL refused two ranks on one device:', got[0]['init'])


@pytest.mark.parametrize('mode', ['fp16', 'bf16'])
def test_regrouped_frontend_shadows_follow_the_optimizer(mode):
    """The frontend's channel-last weight images (nn.ConvFrontEnd.regrouped_weights: conv2's taps, the output Linear's columns,
    frontend/conv.py:141-145) are kept by FlatDataParallel's one transpose launch per optimizer step instead of a copy per forward
    pass: same loss and gradients as the stand-alone module that regroups on the fly, and still right after an update."""
    import copy
    import opentransformer_amd as ota
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    ops.set_compute_dtype(mode)
    try:
        cfg = syn.c1_model(0.0)
        plain = ota.SpeechToText(cfg)
        syn.fill_state_dict_(plain.state_dict(), 5)
        plain = plain.to('cuda').train()
        model = copy.deepcopy(plain)
        dp = FlatDataParallel(model)
        opt = FusedAdam(dp, lr=1e-2, loss_scale=(256.0 if mode == 'fp16' else None))
        fe = model.frontend

        def check_views():
            seen = 0
            for w, (A, R, S) in fe.regrouped_weights():
                v = ops.regrouped_lp(w, (A, S, R))
                assert v is not None, 'no regrouped shadow registered'
                assert torch.equal(v, ops.weight_lp(w).reshape(A, R, S).transpose(1, 2))
                seen += 1
            assert seen == 2
        check_views()
        inputs, targets = syn.synthetic_batch(**BATCH)
        inputs, targets = {k: v.cuda() for k, v in inputs.items()}, {k: v.cuda() for k, v in targets.items()}
        recs = []
        ops.set_kernel_timer(recs)
        try:
            dp.zero_grad()
            loss, _ = dp(inputs, targets)
        finally:
            ops.set_kernel_timer(None)
        ops.backward(loss)
        plain._otr_loss_scale = getattr(model, '_otr_loss_scale', None)     # the same seed scale for both backward passes
        ref, _ = plain(inputs, targets)
        ref.backward()
        ls = float(opt.state[6]) or 1.0
        assert abs(loss.item() - ref.item()) < 1e-3 * abs(ref.item())
        for (n, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
            if n.startswith('frontend'):
                a, b = p.grad.double() / ls, q.grad.double() / ls
                assert float((a - b).norm() / (b.norm() + 1e-30)) < 2e-2, n
        dp.all_reduce_gradients()
        opt.step(1.0)
        torch.cuda.synchronize()
        check_views()                                   # refreshed behind the update
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('V', [4234, 100])
def test_output_layer_on_row_padded_operands(V):
    """A Linear whose width is not a multiple of 8 (the 4234-token output layer, decoder/transformer.py:153) under
    FlatDataParallel: weight, transposed shadow and gradient carry zero rows up to the next multiple of 8 inside the layer's slot of
    the flat buffers, logits and their gradient travel as heads of [R, V8] buffers (otr_label_smoothing_loss_ld), and the three
    GEMMs of the layer run at the padded width.  Same loss and gradients as the unpadded path; the padding stays zero."""
    import copy
    import opentransformer_amd.nn as onn
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(V)
            self.output_layer = torch.nn.Linear(256, V)
            self.crit = onn.LabelSmoothingLoss(V, 0.1)

        def forward(self, x, tgt):
            return self.crit(ops.linear(x, self.output_layer.weight, self.output_layer.bias), tgt)

    ops.set_compute_dtype('fp16')
    try:
        g = torch.Generator().manual_seed(1)
        x0 = torch.randn(32, 15, 256, generator=g).cuda()
        tgt = torch.randint(1, V, (32, 15), generator=g).cuda()
        tgt[3, 9:] = 0                                         # PAD rows
        V8 = (V + 7) // 8 * 8
        res = {}
        for name, on in (('padded', True), ('plain', False)):
            m = Head().cuda().train()
            dp = FlatDataParallel(m)
            w, b = m.output_layer.weight, m.output_layer.bias
            assert tuple(w._otr_pad['param'].shape) == (V8, 256) and tuple(b._otr_pad['param'].shape) == (V8,)
            assert w._otr_pad['param'].data_ptr() == w.data_ptr() and not w._otr_pad['param'][V:].any()
            was = ops._PAD_ROWS
            ops._PAD_ROWS = on
            recs = []
            try:
                x = x0.clone().requires_grad_(True)
                dp.zero_grad()
                ops.set_kernel_timer(recs)
                loss = dp(x, tgt)
                ops.set_kernel_timer(None)
                ops.backward(loss)
                torch.cuda.synchronize()
            finally:
                ops.set_kernel_timer(None)
                ops._PAD_ROWS = was
            names = ' '.join(str(r[0] if isinstance(r, (tuple, list)) else r) for r in recs)
            assert ('linear_fwd 480x%dx256' % (V8 if on else V)) in names, names
            res[name] = (loss.item(), x.grad.clone(), w.grad.clone(), b.grad.clone())
            assert not w._otr_pad['grad'][V:].any() and not b._otr_pad['grad'][V:].any()
            assert not w._otr_pad['lpt'][:, V:].any()
            assert torch.equal(w._otr_pad['lpt'][:, :V], ops.weight_lp(w).t())
            if on:                                              # an update leaves the padding at zero and the shadows in step
                opt = FusedAdam(dp, lr=1e-2, loss_scale=None)
                dp.all_reduce_gradients()
                opt.step(1.0)
                torch.cuda.synchronize()
                assert not w._otr_pad['param'][V:].any() and not b._otr_pad['param'][V:].any()
                assert torch.equal(w._otr_pad['lpt'][:, :V], ops.weight_lp(w).t()) and not w._otr_pad['lpt'][:, V:].any()
        (la, xa, wa, ba), (lb, xb, wb, bb) = res['padded'], res['plain']
        assert abs(la - lb) < 1e-5 * abs(lb)

        def rel(a, b):
            return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
        assert rel(xa, xb) < 2e-3 and rel(wa, wb) < 2e-3 and rel(ba, bb) < 1e-4, (rel(xa, xb), rel(wa, wb), rel(ba, bb))
    finally:
        ops.set_compute_dtype('bf16')


@pytest.mark.parametrize('case', ['c2/fp16/early', 'c2/bf16/single', 'conformer/fp16/early', 'conformer/bf16/single'])
def test_installed_layout_is_the_planned_one(case):
    """What FlatDataParallel installs on the GPU is what its pure plan (dp._plan) says: every _otr_* view by offset from its
    buffer's base, shape and stride, the two device tables element for element -- and both are the layout recorded from the
    commit before the plan (tests/golden/dp_layout.json)."""
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel
    ops.set_compute_dtype(case.split('/')[1])
    try:
        model, early = H.dp_layout_model(case)
        dp = FlatDataParallel(model.to('cuda').train(), early_modules=early)
        try:
            plan = dp._plan
            got, planned = H.dp_installed_layout(dp), H.dp_planned_layout(plan, [tuple(p.shape) for p in dp.params])
            for k in planned:
                assert got[k] == planned[k], k
            assert torch.equal(dp._lpt_table.cpu(), torch.tensor(plan.lpt_table, dtype=torch.int64).reshape(-1, 4))
            assert dp._lpt_tiles == plan.lpt_tiles and dp._pack_blocks == plan.pack_blocks
            if plan.pack_table:
                assert torch.equal(dp._pack_table.cpu(), torch.tensor(plan.pack_table, dtype=torch.int64))
                assert dp.flat_pack.numel() == plan.pack_len
            else:
                assert dp._pack_table is None and dp.flat_pack is None
            H.check_dp_layout(got, H.dp_layout_golden()['device'][case])
        finally:
            dp.close()
            ops.set_early_callback(None)
    finally:
        ops.set_compute_dtype('bf16')
