"""CPU (-m "not gpu"): pins tests/optim_ref.py, the float64 restatement the GPU tests of otr_optimizer_step measure the kernels against
(tests/test_gpu_optimizer.py) -- against the reference's recorded optimizer loop, against torch's own clip_grad_norm_ + Adam in
float64, and, for the dynamic loss scale that torch has no counterpart of, against expectations written out by hand."""
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as ref
from tests.test_gpu_ops import optimizer_inputs

U = 2.0 ** -24                       # unit roundoff of float32


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def test_restatement_matches_the_recorded_reference_loop(golden):
    """tests/golden/optimizer_steps.npz is the reference's TransformerScheduler + torch.optim.Adam loop in float32 over 7 steps (step 2
    clipped, step 4 a NaN that is skipped); the restatement runs the same inputs in float64.

    Bounds (none of them fitted): the recorded float32 parameters round p once per applied update (6 x U of |p|) and each of their
    updates carries the two dozen roundings of torch's element-wise Adam, on an update that is at most lr x (1 - b1) / sqrt(1 - b2) x
    sqrt(bc2) / bc1 < 3.2 x lr in size -- so |p64 - p32| <= 6 U |p| + 24 U x 3.2 x sum(lr) = U (6 |p| + 77 sum(lr)).  The recorded norm
    is a float32 sum of 2 607 squares in 4 tensors: at most log2(2607) + 4 < 16 roundings deep in torch's blocked summation, halved by
    the square root, plus the root, the squares and the norm of the four norms: 16 U.  lr is float64 on both sides: 1e-14.
    Measured: the worst parameter uses 0.14 of its bound (2.8 U of |p| + sum(lr)), the norm 2.2 U, lr agrees to the last bit."""
    g = golden('optimizer_steps.npz')
    shapes, params, grads, hp = optimizer_inputs()
    noam = dict(model_size=hp['model_size'], warmup=hp['warmup_steps'], factor=hp['factor'], step_offset=2.0)
    p = flat(params).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    st = ref.new_state()
    lr_sum, worst_p, worst_n, worst_lr, skipped = 0.0, 0.0, 0.0, 0.0, 0
    for k, gs in enumerate(grads):
        p, m, v, applied = ref.step(p, flat(gs), m, v, st, base_lr=hp['lr'], betas=hp['betas'], eps=hp['eps'],
                                    weight_decay=hp['weight_decay'], clip=hp['clip'], noam=noam)
        assert applied == (not g['skipped'][k]), k
        skipped += int(not applied)
        assert st['skipped'] == skipped == int(g['skipped'][:k + 1].sum()) and st['step'] == k + 1 - skipped
        lr_sum += st['lr'] if applied else 0.0
        want = torch.from_numpy(g['params_%d' % k]).double()
        worst_p = max(worst_p, float(((p - want).abs() / (U * (6 * want.abs() + 77 * lr_sum))).max()))
        worst_lr = max(worst_lr, abs(st['lr'] - float(g['lr'][k])) / float(g['lr'][k]))     # a skipped call keeps the last lr
        norm = math.sqrt(st['sqnorm']) * st['unscale']
        if applied:
            worst_n = max(worst_n, abs(norm - float(g['grad_norm'][k])) / float(g['grad_norm'][k]))
        else:
            assert math.isnan(norm) and math.isnan(float(g['grad_norm'][k]))
    print('optim_ref vs optimizer_steps.npz: parameters %.3f of their bound, norm %.2f U, lr %.1e' % (worst_p, worst_n / U, worst_lr))
    assert skipped == 1 and not g['skipped'][2] and g['grad_norm'][2] > 100 * hp['clip']       # the fixture clips and skips
    assert worst_p <= 1, worst_p
    assert worst_n <= 16 * U, worst_n / U
    assert worst_lr <= 1e-14, worst_lr


def test_restatement_matches_torch_adam_in_float64():
    """clip_grad_norm_ + torch.optim.Adam (L2 weight decay 1e-2, constant lr) in float64, 6 steps, n = 1027 (n % 4 == 3), one step with a
    gradient far above the clip: both sides are float64 evaluations of the same formulas in slightly different operation order, a
    few dozen roundings of 1.1e-16 each -- 1e-12 of (|value| + scale) leaves two orders of room and is eight orders below float32."""
    n, lr, betas, eps, wd, clip = 1027, 1e-3, (0.9, 0.98), 1e-9, 1e-2, 5.0
    gen = torch.Generator().manual_seed(7)
    p0 = 0.3 * torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [(400.0 if k == 3 else 0.05) * torch.randn(n, generator=gen, dtype=torch.float64) for k in range(6)]
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v, st = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), ref.new_state()
    for k, g in enumerate(grads):
        tp.grad = g.clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_([tp], clip))
        opt.step()
        p, m, v, applied = ref.step(p, g, m, v, st, base_lr=lr, betas=betas, eps=eps, weight_decay=wd, clip=clip)
        assert applied and st['step'] == k + 1 and st['lr'] == lr
        assert abs(math.sqrt(st['sqnorm']) - tnorm) <= 1e-12 * tnorm
        ts = opt.state[tp]
        for name, got, want, scale in (('p', p, tp.detach(), 0.3), ('m', m, ts['exp_avg'], 5e-3), ('v', v, ts['exp_avg_sq'], 5e-5)):
            err = float(((got - want).abs() / (want.abs() + scale)).max())
            assert err <= 1e-12, (k, name, err)
    assert (math.sqrt(ref.sqnorm(grads[3])) > 100 * clip) and (math.sqrt(ref.sqnorm(grads[0])) < clip)   # clipped once, else not


HP = dict(base_lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-2, grad_scale=0.25, clip=5.0,
          noam=dict(model_size=256.0, warmup=4.0, factor=1.0, step_offset=2.0))

# the loss-scale transitions, shared with the device test (tests/test_gpu_optimizer.py): name -> (initial loss scale, growth interval,
# [call is finite?], [(loss_scale, good_steps, step, skipped) expected after each call]) -- written out by hand from
# include/otrans_hip.h: a non-finite norm halves the scale (floor 1) and restarts the count; `growth_interval` finite updates in a row
# double it (cap 65536) and restart the count; only applied updates advance the step
TRANSITIONS = {
    'floor': (2.0, 0.0, [False, False], [(1.0, 0, 0, 1), (1.0, 0, 0, 2)]),
    'cap': (32768.0, 1.0, [True, True], [(65536.0, 0, 1, 0), (65536.0, 0, 2, 0)]),
    'restart': (64.0, 3.0, [True, True, False, True, True, True],
                [(64.0, 1, 1, 0), (64.0, 2, 2, 0), (32.0, 0, 2, 1), (32.0, 1, 3, 1), (32.0, 2, 4, 1), (64.0, 0, 5, 1)]),
}


def transition_gradient(n, k, finite, loss_scale):
    """the stored gradient of call k: the true one times loss_scale / grad_scale, a NaN in the last element of a non-finite call"""
    g = 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(100 + k)) * (loss_scale / HP['grad_scale'])
    if not finite:
        g[n - 1] = float('nan')
    return g


@pytest.mark.parametrize('name', sorted(TRANSITIONS))
def test_loss_scale_transitions_by_hand(name):
    ls0, growth, finite, expect = TRANSITIONS[name]
    n = 11
    p = 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    m, v, st = torch.zeros_like(p), torch.zeros_like(p), ref.new_state(ls0, growth)
    for k, (fin, (ls, good, t, skipped)) in enumerate(zip(finite, expect)):
        before, ls_in = (p.clone(), m.clone(), v.clone(), st['lr'], st['bc1'], st['bc2']), st['loss_scale']
        p, m, v, applied = ref.step(p, transition_gradient(n, k, fin, ls_in), m, v, st, **HP)
        assert applied == fin
        assert (st['loss_scale'], st['good_steps'], st['step'], st['skipped']) == (ls, good, t, skipped), (k, st)
        assert st['unscale'] == HP['grad_scale'] / ls_in and st['growth_interval'] == growth   # the scale the gradient CAME with
        if fin:
            assert st['lr'] == ref.noam_lr(t + 2.0, 256.0, 4.0, 1.0) and st['bc1'] == 1 - 0.9 ** t and st['bc2'] == 1 - 0.98 ** t
            assert not torch.equal(p, before[0])
        else:                                        # a skipped call advances neither t nor lr, and touches nothing else
            assert (st['lr'], st['bc1'], st['bc2']) == before[3:]
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
    assert ref.noam_lr(3.0, 256.0, 4.0, 1.0) == 3.0 / (16.0 * 8.0)           # warm-up branch: s * warmup^-1.5 / sqrt(model_size)
    assert ref.noam_lr(16.0, 256.0, 4.0, 1.0) == 1.0 / (16.0 * 4.0)          # decay branch: 1 / sqrt(s * model_size)


def test_launch_arithmetic_of_the_device_test():
    """the seams of the kernels' loops as tests/test_gpu_optimizer.py computes them (from n, the 512-workgroup cap and the block size),
    against the same indices worked out by hand: a wrong index there would test the wrong element and pass"""
    from tests.test_gpu_optimizer import ADAM_WG, BLOCK, corner_indices, norm_launch, sqnorm_depth
    assert norm_launch(1575974) == (393993, 512, 131072) and 393993 == 3 * 131072 + 777
    c = corner_indices(1575974)          # threads i0 < 777 run one unrolled round, the split falls inside workgroup 3
    assert c['last float4 of the unrolled loop'] // 4 == 776 + 3 * 131072 and c['first float4 of the remainder loop'] // 4 == 777
    assert 777 // BLOCK == 3 and 777 % BLOCK != 0 and c['tail element 1'] == 1575973 and 'tail element 2' not in c
    c = corner_indices(2097159)          # every thread once through the unrolled loop, thread 0 once more
    assert c['last float4 of the unrolled loop'] // 4 == 4 * 131072 - 1 and c['first float4 of the remainder loop'] // 4 == 4 * 131072
    assert c['last whole float4'] // 4 == 4 * 131072 and c['tail element 2'] == 2097158
    assert corner_indices(3) == {'tail element 0': 0, 'tail element 1': 1, 'tail element 2': 2}
    assert norm_launch(524288)[1:] == (512, 131072) and norm_launch(524288 - 1024)[1] == 511
    n4 = 5767191 // 4                    # two unrolled rounds, three remainder rounds for threads < 5; adam_kernel: a second pass
    assert n4 == 11 * 131072 + 5 and 5767191 % 4 == 3 and ADAM_WG * BLOCK < n4 < 2 * ADAM_WG * BLOCK
    assert sqnorm_depth(5767191) == 1 + 48 + 1 + 6 + 3 + 8 + 6 and sqnorm_depth(3) == 1 + 0 + 1 + 6 + 3 + 1 + 6
