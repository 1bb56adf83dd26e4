"""Plain float64 restatement of ONE otr_optimizer_step call (include/otrans_hip.h; csrc/optim.hip), laid out like the three launches it
restates so that a test can compare each of them on its own:

  sqnorm(grad)                      the sum of squares of the gradient as it sits in memory           (sqnorm_kernel)
  tick(state, sq, ...)              NaN guard, dynamic loss scale, update count, bias corrections, lr  (opt_tick_kernel)
  adam(p, g, m, v, state, ...)      clip, L2 weight decay, the Adam moments, the parameter update      (adam_kernel)
  step(...)                         the three in a row = one call

`state` is a dict with the first ten slots of the device state block, in the order of STATE.  Tensors are torch float64 on the CPU;
whatever is passed in is widened, never modified.  Gradient noise and the fault word of otr_set_fault_counter are not restated
(noise has a statistical test of its own; a call with grad_noise_std = 0 and no give-up is what this describes).  float64 has no
float32 overflow: a gradient whose sum of squares exceeds 3.4e38 skips on the device and does not here."""
import math

import torch

STATE = ('step', 'lr', 'bc1', 'bc2', 'sqnorm', 'skipped', 'loss_scale', 'good_steps', 'unscale', 'growth_interval')
LOSS_SCALE_MIN, LOSS_SCALE_MAX = 1.0, 65536.0
CLIP_EPS = 1e-6                      # torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6)


def new_state(loss_scale=0.0, growth_interval=0.0):
    """the zero-initialised block; the caller sets slot 6 (loss scale, 0 = off) and slot 9 (growth interval, 0 = never grow)"""
    st = dict.fromkeys(STATE, 0.0)
    st['loss_scale'], st['growth_interval'] = float(loss_scale), float(growth_interval)
    return st


def state_vector(st):
    return [float(st[k]) for k in STATE]


def sqnorm(grad):
    g = torch.as_tensor(grad).double().reshape(-1)
    return float((g * g).sum())                       # a NaN or an infinity anywhere makes it non-finite


def noam_lr(s, model_size, warmup, factor):
    return factor * model_size ** -0.5 * min(s ** -0.5, s * warmup ** -1.5)


def tick(st, sq, base_lr, betas, grad_scale=1.0, noam=None):
    """advance `st` in place by one call whose gradient has the sum of squares `sq`; True when the update is applied.
    noam: None (constant base_lr) or dict(model_size, warmup, factor, step_offset); warmup <= 0 selects base_lr too."""
    st['sqnorm'] = sq
    scaling = st['loss_scale'] > 0
    ls = st['loss_scale'] if scaling else 1.0
    st['unscale'] = grad_scale / ls
    norm = math.sqrt(sq) * st['unscale'] if sq == sq else float('nan')
    if not math.isfinite(norm):                       # skipped: the counters below, the moments and the parameters stay
        st['skipped'] += 1
        if scaling:
            st['loss_scale'] = max(ls / 2, LOSS_SCALE_MIN)
            st['good_steps'] = 0.0
        return False
    if scaling:
        st['good_steps'] += 1
        if st['growth_interval'] > 0 and st['good_steps'] >= st['growth_interval']:
            st['loss_scale'] = min(2 * ls, LOSS_SCALE_MAX)
            st['good_steps'] = 0.0
    st['step'] += 1                                   # Adam's t counts APPLIED updates only
    t = st['step']
    st['bc1'] = 1 - betas[0] ** t
    st['bc2'] = 1 - betas[1] ** t
    if noam is not None and noam['warmup'] > 0:
        st['lr'] = noam_lr(t + noam.get('step_offset', 0.0), noam['model_size'], noam['warmup'], noam['factor'])
    else:
        st['lr'] = base_lr
    return True


def clip_coef(st, clip):
    """what every gradient element is multiplied by: the unscale factor times clip_grad_norm_'s coefficient"""
    norm = math.sqrt(st['sqnorm']) * st['unscale']
    return st['unscale'] * (min(1.0, clip / (norm + CLIP_EPS)) if clip > 0 else 1.0)


def adam(p, g, m, v, st, betas, eps, weight_decay=0.0, clip=0.0):
    """the element-wise part of an APPLIED update, from the scalars tick() left in `st` -> new (p, m, v)"""
    p, g, m, v = (torch.as_tensor(x).double() for x in (p, g, m, v))
    gi = g * clip_coef(st, clip) + weight_decay * p
    m = betas[0] * m + (1 - betas[0]) * gi
    v = betas[1] * v + (1 - betas[1]) * gi * gi
    p = p - (st['lr'] / st['bc1']) * m / (v.sqrt() / math.sqrt(st['bc2']) + eps)
    return p, m, v


def step(p, g, m, v, st, base_lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.0, grad_scale=1.0, clip=0.0, noam=None):
    """one otr_optimizer_step call: advances `st` in place -> (p, m, v, applied); a skipped call returns p, m, v as they came"""
    if not tick(st, sqnorm(g), base_lr, betas, grad_scale, noam):
        return p, m, v, False
    return adam(p, g, m, v, st, betas, eps, weight_decay, clip) + (True,)
