"""GPU (-m gpu): otr_optimizer_step (csrc/optim.hip: sqnorm_kernel -> opt_tick_kernel -> adam_kernel) through the C ABI on caller-owned,
guarded buffers, at the sizes where its launch arithmetic changes, in both 16-bit builds, against the float64 restatement of
tests/optim_ref.py (pinned on the CPU by tests/test_optim_ref.py).

Each launch is measured on its own, on the float32 values it actually read, widened to float64 -- U = 2^-24, float32's unit roundoff:

* sqnorm_kernel + the tick kernel's fixed-order sum (state[4]) against the float64 sum of squares.  All terms are >= 0, so the relative
  error is at most (longest chain of roundings one term passes through) x U: `sqnorm_depth`.
* opt_tick_kernel (state[0..9]) against optim_ref.tick fed the float64 sum.  Counters, the loss scale and the unscale factor (a quotient
  of powers of two) are exact.  lr = factor * rsqrtf(model) * fminf(rsqrtf(s), s * powf(warmup, -1.5)): rsqrtf and powf are good to
  1 ulp = 2 U each (HIP math API), three products: 2 + 1 + max(2, 2 + 1) + 1 = 7 U relative.  bc = 1 - powf(beta, t): 2 U of
  beta^t < 1 plus the subtraction's U of bc < 1: 3 U ABSOLUTE.
* adam_kernel element by element against optim_ref.adam fed the scalars the kernel read (state[1..4], state[8] after the call) and
  p, m, v from before the call.  Roundings, counted in the code: coef = us * fminf(1, clip / (sqrtf(sqnorm) * us + 1e-6f)) 5, and the
  float32 constant 1e-6f for a 6th; g * coef 1; wd * p 1; their sum 1; m: beta1 * m, (1 - beta1), * g', the sum: 3 on either
  term; v: (1 - beta2), two products with g', beta2 * v, the sum: 4; the denominator: sqrtf 1, rsqrtf(bc2) 2, the product 1, + eps 1:
  5; the update: lr / bc1, * m, / denominator: 3; p - update 1.  For an element without cancellation that is
  (6 + 1 + 1) + 3 = 11 U on m, 2 x 8 + 4 = 20 U on v, and 11 + (20 / 2 + 5) + 3 = 29 U on the update d = p_new - p_old, plus U on |p|:
      |got - ref| <= U |p| + 29 U |d|
  (d ~ lr ~ 1e-3: about 2e-9; an element that was skipped or updated twice is off by |d|, five orders more).  g' = g * coef + wd * p
  and beta1 * m + (1 - beta1) * g' DO cancel in a few elements of millions, so the test propagates the same counts as intervals
  (`adam_bounds`) instead of multiplying them onto |ref|: where nothing cancels the interval IS the line above -- the test asserts
  that on every element whose two sums are conditioned within 1 + 1/16 its half-width, less U |p|, stays under 32 U |d| -- and
  where g' all but cancels it widens to what the float32 evaluation can really give.
* the 16-bit shadow is bit-equal to the rounded float32 parameter over all n; every buffer carries 64 sentinel elements in front of
  element 0 and behind element n - 1, untouched after every call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as ref
from tests.test_optim_ref import HP, TRANSITIONS, transition_gradient

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
TINY = 2.0 ** -126                   # below the smallest normal float32 nothing is promised (denormals may flush)
GUARD = 64                           # elements: 256 bytes of float32, 128 of the 16-bit type -- the 16-byte alignment survives
BLOCK, NORM_WG, ADAM_WG = 256, 512, 4096          # csrc/optim.hip: threads per workgroup, grid caps of sqnorm_kernel / adam_kernel
LR_ULPS, BC_ULPS = 7, 3
C_COEF, C_M, C_V, C_DEN, C_UPD = 6, 3, 4, 5, 3    # roundings, see the module docstring


def f32(x):
    """the float32 the C ABI turns a Python float into, widened back: the reference gets the hyper-parameters the kernel got"""
    return float(np.float32(x))


def hp32(hp):
    return {k: (tuple(f32(b) for b in v) if k == 'betas' else f32(v) if k != 'noam' else v and {a: f32(b) for a, b in v.items()})
            for k, v in hp.items()}


@pytest.fixture(params=['bf16', 'fp16'])
def build(request):
    """both libraries: they differ in the conversion that writes the 16-bit shadow"""
    from opentransformer_amd import ops
    ops.set_compute_dtype(request.param)
    try:
        yield request.param
    finally:
        ops.set_compute_dtype('bf16')


# ------------------------------------------------------------------------------------------ launch arithmetic, restated
def norm_launch(n):
    """-> (n4, workgroups of sqnorm_kernel, its grid stride in float4)"""
    n4 = n // 4
    grid = max(1, min((n4 + BLOCK - 1) // BLOCK, NORM_WG))
    return n4, grid, grid * BLOCK


def sqnorm_depth(n):
    """longest chain of float32 roundings between one g[i] and state[4]: its square; per float4 of its thread three adds inside the
    float4 and one onto the running sum (4 x ceil(n4 / stride), rounded up); the tail element's add; the 6-step butterfly; 3 adds in
    LDS; in the tick kernel ceil(workgroups / 64) serial adds and another butterfly"""
    n4, grid, stride = norm_launch(n)
    return 1 + 4 * ((n4 + stride - 1) // stride) + 1 + 6 + 3 + (grid + 63) // 64 + 6


def corner_indices(n):
    """element indices at the seams of sqnorm_kernel's loops, from n, the 512-workgroup cap and the block size, as the kernel computes
    them: {name: element index}.  Thread i0 runs k unrolled rounds over float4 i0 + (4 r + j) stride, then the remainder loop from
    i0 + 4 k stride in steps of stride; workgroup 0 takes the n & 3 tail elements."""
    n4, grid, stride = norm_launch(n)
    out = {}
    i0 = np.arange(min(stride, max(n4, 1)), dtype=np.int64)
    k = np.where(i0 + 3 * stride < n4, (n4 - 1 - i0 - 3 * stride) // (4 * stride) + 1, 0)
    if (k > 0).any():
        out['last float4 of the unrolled loop'] = int((i0 + (4 * k - 1) * stride)[k > 0].max())
    rem = i0 + 4 * k * stride
    if (rem < n4).any():
        out['first float4 of the remainder loop'] = int(rem[rem < n4].min())
    if n4:
        out['last whole float4'] = n4 - 1
    el = {name: 4 * f + (f & 3) for name, f in out.items()}             # some lane of that float4
    for j in range(n & 3):
        el['tail element %d' % j] = 4 * n4 + j
    return el


# ------------------------------------------------------------------------------------------ guarded buffers and the call
class Guarded:
    """n elements with GUARD sentinel elements on either side"""

    def __init__(self, n, dtype, sentinel):
        self.store = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        self.t = self.store[GUARD:GUARD + n]
        self.front, self.back = self.store[:GUARD].clone(), self.store[GUARD + n:].clone()
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return torch.equal(self.store[:GUARD], self.front) and torch.equal(self.store[GUARD + self.t.numel():], self.back)


class Call:
    """caller-owned buffers of one parameter vector of n elements, and the reference's state next to the device's"""

    def __init__(self, n, p0, loss_scale=0.0, growth=0.0, m0=None, v0=None):
        from opentransformer_amd import _lib, ops
        self.n, self.lib, self.L = n, _lib.load(), _lib
        self.buf = {k: Guarded(n, torch.float32, 12345.0) for k in 'pgmv'}
        self.buf['s'] = Guarded(_lib.OTR_OPT_STATE_FLOATS, torch.float32, 12345.0)
        self.buf['h'] = Guarded(n, ops.half_dtype(), 77.0)
        self.p, self.g, self.m, self.v, self.state, self.shadow = (self.buf[k].t for k in 'pgmvsh')
        self.p.copy_(p0)
        self.m.copy_(m0) if m0 is not None else self.m.zero_()
        self.v.copy_(v0) if v0 is not None else self.v.zero_()
        self.shadow.copy_(self.p.to(self.shadow.dtype))
        self.state.zero_()
        self.state[6], self.state[9] = loss_scale, growth
        self.ref = ref.new_state(loss_scale, growth)

    def launch(self, grad, hp):
        """one otr_optimizer_step on the stored gradient `grad` (CPU float32) -> the state block after it, as float64 list"""
        self.g.copy_(grad)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        nm = hp['noam'] or dict(model_size=1.0, warmup=0.0, factor=1.0, step_offset=0.0)
        ret = self.lib.otr_optimizer_step(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), self.n, ptr(self.state),
                                          self.L.OTR_OPT_STATE_FLOATS, ptr(self.shadow), hp['base_lr'], hp['betas'][0], hp['betas'][1],
                                          hp['eps'], hp['weight_decay'], hp['grad_scale'], hp['clip'], nm['model_size'], nm['warmup'],
                                          nm['factor'], nm['step_offset'], 0.0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.L.check(ret, 'otr_optimizer_step')
        torch.cuda.synchronize()
        for k, b in self.buf.items():
            assert b.intact(), 'guard band of buffer %r overwritten (n = %d)' % (k, self.n)
        assert torch.equal(self.g.view(torch.int32).cpu(), grad.view(torch.int32)), 'the gradient is an input'
        return self.state[:16].double().tolist()

    def step(self, grad, hp, what='', share=False):
        """one call, every launch of it against the reference (module docstring) -> True when the update was applied"""
        before = [t.to('cpu', copy=True) for t in (self.p, self.m, self.v, self.shadow)]
        dev = self.launch(grad, hp)
        applied = check_tick(self.ref, dev, grad, self.n, hp, what)
        after = [t.to('cpu', copy=True) for t in (self.p, self.m, self.v, self.shadow)]
        if applied:
            check_adam(before[:3], grad, after[:3], dev, hp, norm_launch(self.n)[2], what, share)
            assert torch.equal(after[3], after[0].to(after[3].dtype)), (what, 'shadow != rounded parameter')
        else:
            for name, a, b in zip('pmvh', before, after):
                assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                   b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), (what, name, 'changed by a skipped call')
        return applied


def check_tick(rst, dev, grad, n, hp, what=''):
    """state[0..9] after a call against optim_ref.tick on the float64 sum of squares; advances `rst` -> applied?"""
    sq = ref.sqnorm(grad)
    applied = ref.tick(rst, sq, hp['base_lr'], hp['betas'], hp['grad_scale'], hp['noam'])
    want = ref.state_vector(rst)
    depth = sqnorm_depth(n)
    if math.isfinite(sq):
        assert abs(dev[4] - sq) <= depth * U * sq, (what, 'sqnorm', dev[4], sq, abs(dev[4] - sq) / (U * sq), depth)
    else:
        assert not math.isfinite(dev[4]), (what, 'sqnorm', dev[4], sq)
    for i in (0, 5, 6, 7, 8, 9):                       # counters, loss scale, unscale (quotient of powers of two): exact
        assert dev[i] == want[i], (what, ref.STATE[i], dev[i], want[i], dev[:10], want)
    assert abs(dev[1] - want[1]) <= LR_ULPS * U * want[1], (what, 'lr', dev[1], want[1])
    for i in (2, 3):
        assert abs(dev[i] - want[i]) <= BC_ULPS * U, (what, ref.STATE[i], dev[i], want[i])
    return applied


def adam_bounds(p, g, m, v, s, hp):
    """intervals the float32 evaluation of adam_one must land in, around optim_ref.adam on the same scalars: the rounding counts of
    the module docstring, propagated.  float64 tensors -> (m_lo, m_hi, v_lo, v_hi, p_lo, p_hi)"""
    b1, b2 = hp['betas']
    a, b = g * ref.clip_coef(s, hp['clip']), hp['weight_decay'] * p
    gi = a + b
    e_g = U * ((C_COEF + 2) * a.abs() + 2 * b.abs())                   # coef, g * coef, the sum | wd * p, the sum
    m_new = b1 * m + (1 - b1) * gi
    e_m = (1 - b1) * e_g + C_M * U * (b1 * m.abs() + (1 - b1) * gi.abs())
    sq_hi, sq_lo = (gi.abs() + e_g) ** 2, (gi.abs() - e_g).clamp_(min=0) ** 2
    v_hi = (b2 * v + (1 - b2) * sq_hi) * (1 + C_V * U) + TINY
    v_lo = ((b2 * v + (1 - b2) * sq_lo) * (1 - C_V * U) - TINY).clamp_(min=0)
    rbc2, step_size = 1 / math.sqrt(s['bc2']), s['lr'] / s['bc1']
    d_hi = (v_hi.sqrt() * rbc2 + hp['eps']) * (1 + C_DEN * U)
    d_lo = (v_lo.sqrt() * rbc2 + hp['eps']) * (1 - C_DEN * U)
    m_hi, m_lo = m_new + e_m + TINY, m_new - e_m - TINY
    q_hi, q_lo = torch.maximum(m_hi / d_lo, m_hi / d_hi), torch.minimum(m_lo / d_lo, m_lo / d_hi)
    slack = C_UPD * U * step_size * torch.maximum(q_hi.abs(), q_lo.abs())
    p_hi, p_lo = p - step_size * q_lo + slack, p - step_size * q_hi - slack
    last = U * torch.maximum(p_hi.abs(), p_lo.abs())                   # the rounding of p - update
    return m_lo, m_hi, v_lo, v_hi, p_lo - last, p_hi + last


_REFERENCE = {}                      # digest of one call's inputs -> its float64 reference and intervals, kept for the other build


def reference_of_call(before, grad, dev, hp, what, share):
    """optim_ref.adam and the intervals around it for one applied call.  The float64 passes over millions of elements are the
    cost of this module, and the two builds run the same float32 arithmetic on the same inputs: a test that runs in both
    (`share`) keeps the result, from 2^20 elements on, under a digest of EVERYTHING it depends on (p, m, v before, the gradient, the state block, the hyper-parameters) and handed
    to the second build -- which gets it only if every one of those bits is the same, and computes its own otherwise."""
    import hashlib
    key = None
    if share and grad.numel() >= 1 << 20:
        h = hashlib.blake2b(repr((dev[:10], sorted(hp.items(), key=repr))).encode())
        for t in (*before, grad):
            h.update(t.contiguous().numpy().tobytes())
        key = h.digest()
        if key in _REFERENCE:
            return _REFERENCE.pop(key)
    s = dict(zip(ref.STATE, dev[:10]))
    p, m, v, g = (t.double() for t in (*before, grad))
    rp, rm, rv = ref.adam(p, g, m, v, s, hp['betas'], hp['eps'], hp['weight_decay'], hp['clip'])
    lo_hi = adam_bounds(p, g, m, v, s, hp)
    for k, want in enumerate((rm, rv, rp)):
        assert bool(((lo_hi[2 * k] <= want) & (want <= lo_hi[2 * k + 1])).all()), (what, 'mvp'[k], 'the interval lost its own reference')
    # where nothing cancels the interval is the documented line U |p| + 29 U |d|: with both sums conditioned within 1 + 1/16 the counts
    # come to (8.5 + 3) * 1.0625 + (2 * 8.5 + 4) / 2 + 5 + 3 = 30.7 U |d| -- under 32, or the interval above is not the documented one
    a, b = g * ref.clip_coef(s, hp['clip']), hp['weight_decay'] * p
    gi, b1 = a + b, hp['betas'][0]
    d = (rp - p).abs()
    well = (a.abs() + b.abs() <= 1.0625 * gi.abs()) & (b1 * m.abs() + (1 - b1) * gi.abs() <= 1.0625 * rm.abs()) & (d > 0)
    if bool(well.any()):
        c_eff = (((lo_hi[5] - lo_hi[4]) / 2 - U * rp.abs())[well] / (U * d[well])).max()
        assert float(c_eff) <= 32, (what, 'rounding count of the parameter bound where nothing cancels', float(c_eff))
    out = ((rm, rv, rp), lo_hi)
    if key is not None:
        _REFERENCE[key] = out
    return out


def check_adam(before, grad, after, dev, hp, stride, what='', share=False):
    """p, m, v after an applied call, element by element (CPU tensors; dev = the state block after the call)"""
    wants, lo_hi = reference_of_call(before, grad, dev, hp, what, share)
    for k, (name, got, want) in enumerate(zip('mvp', (after[1], after[2], after[0]), wants)):
        lo, hi, got = lo_hi[2 * k], lo_hi[2 * k + 1], got.double()
        out = torch.maximum(got - hi, lo - got)                          # > 0: outside
        i = int(out.argmax())
        assert float(out[i]) <= 0, ('%s: %s[%d] (float4 %d, thread %d of the grid stride %d) = %r, reference %r, allowed [%r, %r]; '
                                    '%d elements outside' % (what, name, i, i // 4, i // 4 % stride, stride, float(got[i]),
                                                             float(want[i]), float(lo[i]), float(hi[i]), int((out > 0).sum())))


# ------------------------------------------------------------------------------------------ a. sizes
SIZES = [
    (1, 2),            # n4 = 0: tail only, grid forced to 1
    (3, 2),            # n4 = 0: tail only, all three tail lanes
    (4, 2),            # one float4, no tail
    (1027, 2),         # two workgroups, tail of 3
    (524288, 2),       # grid exactly at the 512-workgroup cap, one float4 per thread
    (524293, 2),       # cap reached: thread 0 once more in the remainder loop, tail of 1
    (1575974, 2),      # n4 = 3 * 131072 + 777: only threads < 777 enter the unrolled loop, the split inside workgroup 3, tail of 2
    (2097159, 2),      # every thread once through the unrolled loop, thread 0 once more in the remainder loop, tail of 3
    (5767191, 3),      # n4 = 11 * 131072 + 5: two unrolled rounds + three remainder rounds; adam_kernel past its 4096-workgroup cap,
                       # a second pass for part of its grid; tail of 3
]
LOSS_SCALE = 1024.0


def stored_gradient(n, k, gen):
    """fresh gradient of step k as it sits in memory: the true 0.05 * randn times world (1 / grad_scale = 4) times the loss scale;
    step 1 is 400 times larger, so the clip is active in that step and in no other"""
    return 0.05 * torch.randn(n, generator=gen) * (4.0 * LOSS_SCALE * (400.0 if k == 1 else 1.0))


@pytest.mark.parametrize('n,steps', SIZES)
def test_step_matches_reference_at_the_launch_boundaries(build, n, steps):
    hp = hp32(HP)
    gen = torch.Generator().manual_seed(1000 + n % 997)
    call = Call(n, 0.3 * torch.randn(n, generator=gen), loss_scale=LOSS_SCALE)
    clipped = []
    for k in range(steps):
        grad = stored_gradient(n, k, gen)
        assert call.step(grad, hp, 'n=%d step %d %s' % (n, k, build), share=True)
        norm = math.sqrt(call.ref['sqnorm']) * call.ref['unscale']
        clipped.append(norm > hp['clip'])
        assert call.ref['step'] == k + 1 and call.ref['skipped'] == 0 and call.ref['loss_scale'] == LOSS_SCALE
    if n == 1027:        # |0.05 randn(n)| ~ 0.05 sqrt(n): under the clip of 5 up to n ~ 10^4 (above it every step is clipped, step 1 harder;
        assert clipped == [False, True]      # at n <= 4 it is left to the draw) -- here the clip is off in step 0 and on in step 1


# ------------------------------------------------------------------------------------------ c. the norm sees every element
CORNER_SIZES = [1575974, 2097159, 3]


@pytest.mark.parametrize('n', CORNER_SIZES)
def test_norm_sees_every_element(n):
    """an all-zero gradient but for ONE element of 1000 at a seam of the loops: clipped to 5, so exp_avg of that element is
    (1 - beta1) * 5 / (1 + 1e-9) and of every other element exactly 0 (no weight decay).  Roundings on that element: coef 6, g * coef 1,
    m 3 -- 10 U; the norm is a sum of one non-zero term: sqrt exact to the issue's 1e-6."""
    hp = hp32(dict(HP, weight_decay=0.0, grad_scale=1.0, noam=None))
    p0 = 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(5))
    for name, i in corner_indices(n).items():
        call = Call(n, p0)
        grad = torch.zeros(n)
        grad[i] = 1000.0
        dev = call.launch(grad, hp)
        assert abs(math.sqrt(dev[4]) - 1000.0) <= 1e-6 * 1000.0, (n, name, i, dev[4])
        assert dev[0] == 1 and dev[5] == 0
        want = (1 - hp['betas'][0]) * 1000.0 * (hp['clip'] / (1000.0 + 1e-6))
        assert abs(float(call.m[i]) - want) <= 10 * U * want, (n, name, i, float(call.m[i]), want)
        assert int(torch.count_nonzero(call.m)) == 1 and int(torch.count_nonzero(call.v)) == 1, (n, name, i)
        moved = torch.nonzero(call.p != p0.to(DEV)).reshape(-1).tolist()
        assert moved == [i], (n, name, i, moved[:8])
        assert torch.equal(call.shadow, call.p.to(call.shadow.dtype))


# ------------------------------------------------------------------------------------------ d. non-finite values in the corners
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('n', CORNER_SIZES)
def test_non_finite_value_in_a_corner_skips_the_update(n, bad):
    """a NaN / an infinity that sits only at a seam of the loops must still reach the guard: skipped, loss scale 8 -> 4, nothing written
    (Call.step compares p, m, v and the shadow bit for bit); the finite call after it is update t = 1 with the bias correction of a
    first update (checked against the reference like every applied call)"""
    hp = hp32(HP)
    gen = torch.Generator().manual_seed(11)
    p0, m0, v0 = 0.3 * torch.randn(n, generator=gen), 1e-3 * torch.randn(n, generator=gen), 1e-6 * torch.rand(n, generator=gen)
    good = 0.05 * torch.randn(n, generator=gen) * 4.0
    corners = corner_indices(n)
    for name, i in corners.items():
        call = Call(n, p0, loss_scale=8.0, m0=m0, v0=v0)
        grad = good * 8.0
        grad[i] = bad
        assert not call.step(grad, hp, 'n=%d %s at the %s' % (n, bad, name))
        assert (call.ref['skipped'], call.ref['loss_scale'], call.ref['step']) == (1, 4.0, 0)
        dev = call.launch(good * 4.0, hp)              # the gradient now arrives scaled by 4
        assert (dev[0], dev[5], dev[6], dev[7]) == (1, 1, 4.0, 1), (name, dev[:10])
        assert abs(dev[2] - (1 - hp['betas'][0])) <= BC_ULPS * U and abs(dev[3] - (1 - hp['betas'][1])) <= BC_ULPS * U
        assert abs(dev[1] - ref.noam_lr(3.0, 256.0, 4.0, 1.0)) <= LR_ULPS * U * dev[1]
    # the last placement once more, its finite call in full against the reference
    call = Call(n, p0, loss_scale=8.0, m0=m0, v0=v0)
    grad = good * 8.0
    grad[i] = bad
    assert not call.step(grad, hp, 'n=%d %s' % (n, bad))
    assert call.step(good * 4.0, hp, 'n=%d finite call after a skip' % n)
    assert call.ref['step'] == 1 and call.ref['bc1'] == 1 - hp['betas'][0]


# ------------------------------------------------------------------------------------------ e. the loss-scale state machine
@pytest.mark.parametrize('name', sorted(TRANSITIONS))
def test_loss_scale_state_machine_on_the_device(name):
    """the sequences tests/test_optim_ref.py writes out by hand (floor at 1, cap at 65536, a skip restarts the count of good steps),
    n = 1027; state[:10] against the reference after every call, the hand-written expectation next to it"""
    ls0, growth, finite, expect = TRANSITIONS[name]
    n, hp = 1027, hp32(HP)
    call = Call(n, 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(1)), loss_scale=ls0, growth=growth)
    for k, (fin, want) in enumerate(zip(finite, expect)):
        grad = transition_gradient(n, k, fin, call.ref['loss_scale'])
        assert call.step(grad, hp, '%s call %d' % (name, k)) == fin
        dev = call.state[:10].tolist()
        assert (dev[6], dev[7], dev[0], dev[5]) == want, (name, k, dev)


# ------------------------------------------------------------------------------------------ f. through FusedAdam
def test_fused_adam_plumbing_past_the_unrolled_loop():
    """FlatDataParallel + FusedAdam hand the same combination (clip, loss scale, 1 / world, weight decay, Noam) to the entry: one
    parameter of 1 600 000 elements, a flat buffer past the 1 572 864 elements where the unrolled loop of the norm starts"""
    from opentransformer_amd import ops
    from opentransformer_amd.dp import FlatDataParallel, FusedAdam
    n, hp = 1600000, hp32(HP)
    gen = torch.Generator().manual_seed(21)
    p0 = 0.3 * torch.randn(n, generator=gen)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(p0.clone().to(DEV))

    deferral = ops._wq['on']
    try:
        dp = FlatDataParallel(Holder())
        N, off = dp.flat_param.numel(), dp.offsets[0]
        assert N > 1572864 and len(dp.params) == 1
        opt = FusedAdam(dp, lr=HP['base_lr'], betas=HP['betas'], eps=HP['eps'], weight_decay=HP['weight_decay'], clip_grad=HP['clip'],
                        loss_scale=LOSS_SCALE, noam=dict(model_size=256, warmup_steps=4, factor=1.0))
        rst = ref.new_state(LOSS_SCALE, float(opt.state[9]))
        pad = torch.ones(N, dtype=torch.bool)
        pad[off:off + n] = False
        dp.zero_grad()
        for k in range(3):
            dp.params[0].grad.copy_(stored_gradient(n, k, gen).to(DEV))
            grad = dp.flat_grad.cpu()
            before = [t.cpu() for t in (dp.flat_param, opt.exp_avg, opt.exp_avg_sq)]
            assert not bool(grad[pad].any()) and not bool(before[0][pad].any())
            opt.step(grad_scale=HP['grad_scale'])
            torch.cuda.synchronize()
            dev = opt.state.double().tolist()
            assert check_tick(rst, dev, grad, N, hp, 'FusedAdam step %d' % k)
            after = [t.cpu() for t in (dp.flat_param, opt.exp_avg, opt.exp_avg_sq)]
            check_adam(before, grad, after, dev, hp, norm_launch(N)[2], 'FusedAdam step %d' % k)
            assert torch.equal(dp.params[0].detach().reshape(-1).cpu(), after[0][off:off + n])     # the parameter IS the flat slice
            for t in after:
                assert not bool(t[pad].any()), 'padding of the flat buffers must stay exactly zero'
            true_sq = ref.sqnorm(grad.double() / LOSS_SCALE)
            got = opt.stats()['grad_sqnorm']
            assert abs(got - true_sq) <= sqnorm_depth(N) * U * true_sq, (k, got, true_sq)
            assert math.sqrt(true_sq) * HP['grad_scale'] > HP['clip'] * (400 if k == 1 else 1)       # clipped, the second call 400 x harder
            if dp.flat_param_lp is not None:
                assert torch.equal(dp.flat_param_lp.cpu(), after[0].to(dp.flat_param_lp.dtype))
        assert opt.stats()['step'] == 3 and opt.stats()['skipped'] == 0
    finally:
        ops.defer_weight_grads(deferral)
