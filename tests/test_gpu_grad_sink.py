"""GPU (-m gpu): the three functions every backward pass hands its parameter gradients to (ops.sink_wgrad, ops.sink_colsum,
ops.sink_colsum_blocks), each delivered the three ways -- returned to autograd (plain), accumulated into an in-place gradient buffer
now, or queued for the grouped launches at the end of the pass -- from the backward of a tiny autograd Function, so that
ops._in_backward() holds.  fp32 compute mode; every result against the float64 sum within n * 2^-23 * sum |terms| per element (n
terms: the bound of an fp32 sum in any order, with a factor of two for the rounding of the products)."""
import pytest
import torch

from opentransformer_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WAYS = ('plain', 'now', 'deferred')
PREFILL = 0.5            # .grad before an in-place run: a store in place of an add would lose it
ROWS, N, K = 70, 24, 40  # dy [70, 24], x [70, 40]: the rows are no multiple of 32 or 64
PROWS, NBLK = 5, 4       # partial sums: 5 rows, 4 column blocks, of which blocks 0, 1 and 3 are gradients


@pytest.fixture(autouse=True)
def _fp32_mode():
    ops.set_compute_dtype('fp32')
    try:
        yield
    finally:
        ops.defer_weight_grads(False)
        ops.discard_pending_weight_grads()
        ops.set_compute_dtype('bf16')


@pytest.fixture(scope='module')
def data():
    gen = torch.Generator().manual_seed(77)
    dy, x = torch.randn(ROWS, N, generator=gen), torch.randn(ROWS, K, generator=gen)
    parts = {w: torch.randn(PROWS, NBLK * w, generator=gen) for w in (24, 6)}
    d = {'dy': dy, 'x': x, 'parts': parts,
         'w': (dy.double().t() @ x.double(), ROWS * 2.0 ** -23 * (dy.double().abs().t() @ x.double().abs())),
         'b': (dy.double().sum(0), ROWS * 2.0 ** -23 * dy.double().abs().sum(0))}
    for w, p in parts.items():
        d['s', w] = (p.double().sum(0), PROWS * 2.0 ** -23 * p.double().abs().sum(0))
    return d


class _Drive(torch.autograd.Function):
    """identity whose backward runs `fn` inside the autograd pass"""

    @staticmethod
    def forward(ctx, t, fn):
        ctx.fn = fn
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def run_in_backward(fn):
    t = torch.zeros(1, device=DEV, requires_grad=True)
    _Drive.apply(t, fn).sum().backward()
    torch.cuda.synchronize()


def param(shape, way):
    p = torch.zeros(shape, device=DEV, requires_grad=True)
    if way != 'plain':
        p.grad = torch.full(shape, PREFILL, device=DEV)
        p._otr_grad_inplace = True
    return p


def check(way, p, returned, want, bound):
    """None came back exactly when the gradient went in place; the value, wherever it landed, is the float64 sum within the bound"""
    if way == 'plain':
        assert returned is not None and p.grad is None
        got = returned.double().cpu().reshape(want.shape)
    else:
        assert returned is None
        got = p.grad.double().cpu().reshape(want.shape) - PREFILL
    err = (got - want).abs()
    assert bool((err <= bound).all()), (way, float((err / bound).max()))


def queued():
    return len(ops._wq['w']), len(ops._wq['b'])


@pytest.mark.parametrize('way', WAYS)
def test_weight_gradient(data, way):
    dy, x = data['dy'].to(DEV), data['x'].to(DEV)
    p = param((N, K), way)
    ops.defer_weight_grads(way == 'deferred')
    seen = {}

    def fn():
        seen['ret'] = ops.sink_wgrad(dy, x, p)
        seen['queued'] = queued()

    run_in_backward(fn)
    assert seen['queued'] == ((1, 0) if way == 'deferred' else (0, 0))       # queued, not launched, before the pass ends
    assert queued() == (0, 0)
    check(way, p, seen['ret'], *data['w'])


@pytest.mark.parametrize('way', WAYS)
def test_bias_gradient(data, way):
    """... and a parameter that does not exist (None) gets None and launches nothing; defer=False runs now even with deferral on"""
    dy = data['dy'].to(DEV)
    p, q = param((N,), way), param((N,), way)
    ops.defer_weight_grads(way == 'deferred')
    seen = {}

    def fn():
        seen['none'] = ops.sink_colsum(dy, None)
        seen['ret'] = ops.sink_colsum(dy, p)
        seen['queued'] = queued()
        seen['ret_now'] = ops.sink_colsum(dy, q, defer=False)
        seen['queued_now'] = queued()

    run_in_backward(fn)
    assert seen['none'] is None
    assert seen['queued'] == seen['queued_now'] == ((0, 1) if way == 'deferred' else (0, 0))
    check(way, p, seen['ret'], *data['b'])
    check(way, q, seen['ret_now'], *data['b'])


@pytest.mark.parametrize('summed', [False, True])
@pytest.mark.parametrize('width', [24, 6])
@pytest.mark.parametrize('way', WAYS)
def test_partial_sum_blocks(data, way, width, summed):
    """blocks 0, 1 and 3 of four: block 2 belongs to nobody and reaches nobody; a ref of None is skipped.  At width 6 block 1 starts 24
    bytes into a row and block 3 72 bytes: no 16-byte alignment, so the column sum runs now even with deferral on (and the summed form,
    which defers all blocks or none, takes its one-sum path)."""
    part = data['parts'][width].to(DEV)
    want, bound = data['s', width]
    blocks = (0, 1, 3)
    ps = [param((width,), way) for _ in blocks]
    qs = [param((width,), way), None, param((width,), way)]
    ops.defer_weight_grads(way == 'deferred')
    seen = {}

    def fn():
        seen['ret'] = ops.sink_colsum_blocks(part, width, blocks, ps, summed=summed)
        seen['queued'] = queued()
        seen['ret_none'] = ops.sink_colsum_blocks(part, width, blocks, qs, summed=summed)
        seen['queued_none'] = queued()

    run_in_backward(fn)
    aligned = [(part.data_ptr() + 4 * c * width) % 16 == 0 for c in blocks]
    if way != 'deferred' or (summed and width % 4 != 0):
        n_all = n_none = 0
    else:
        n_all, n_none = sum(aligned), aligned[0] + aligned[2]
    assert (width, aligned) in ((24, [True, True, True]), (6, [True, False, False]))
    assert seen['queued'] == (0, n_all) and seen['queued_none'] == (0, n_all + n_none)
    assert len(seen['ret']) == len(seen['ret_none']) == 3 and seen['ret_none'][1] is None
    for c, p, r in zip(blocks, ps, seen['ret']):
        check(way, p, r, want[c * width:(c + 1) * width], bound[c * width:(c + 1) * width])
    for c, q, r in zip(blocks, qs, seen['ret_none']):
        if q is not None:
            check(way, q, r, want[c * width:(c + 1) * width], bound[c * width:(c + 1) * width])
