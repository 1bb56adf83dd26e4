"""GPU (-m gpu): the one backward of the six loss Functions (loss_ops._saved_logits_grad), each reached through its public wrapper, or
directly for CTCLossFn and LabelSmoothingLossFn, at V = 36 on rows of 40 floats (the head of a row-padded buffer) and at V = 40
contiguous, R = 12 rows.

The unit seed of ops.backward against a seed of 2.5, each on fresh inputs.  A backward is otr_scale of the buffer its forward saved, or
that buffer itself.  scale_kernel (csrc/elementwise.hip) forms x[i] * ((*s_dev) * 1.f), one fp32 rounding of the product torch forms
for seed * x, so every gradient equals seed * (the buffer its own forward saved) bit for bit, with zeros behind column V.  Where the
forward writes the same bits on every run, the two gradients are therefore 2.5 apart bit for bit.  The two CTC forwards do not: the
blank column of their gradient collects several atomicAdds per frame in a free order (tests/test_gpu_ctc_loss.py says so of
otr_ctc_loss; in the pair form both label sets add there too), so two launches may differ in that column's last bits before any
backward has run.  For them the 2.5 is asserted across the runs in every other column: the label sets below share no label and repeat
none, so each of those cells takes one add per frame.  And the switch ops._LS_FUSED selects between the two label-smoothing forms."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
R, LD = 12, 40
B, T, W, N, K = 2, 6, 3, 2, 4
WIDTHS = [36, 40]
FREE_ORDER = {'ctc', 'ctc_pair'}                                   # forwards whose blank column is summed by atomics
PADDED = {'ls', 'ls_fused', 'mwer', 'distill', 'distill_topk'}      # these hand a [R, 40] buffer back at V = 36; the CTC pair does not


@functools.lru_cache(maxsize=None)
def _data(V):
    """the inputs every case at this width shares; nothing below writes to them"""
    g = torch.Generator().manual_seed(V)
    d = {'buf': torch.randn(R, LD, generator=g).to(DEV), 'teacher': torch.randn(B, T, V, generator=g).to(DEV),
         'target': torch.randint(1, V, (B, T), generator=g).to(DEV),
         'labels_a': torch.tensor([[3, 5, 7], [2, 4, 0]], device=DEV), 'labels_b': torch.tensor([[9, 1, 0], [6, 8, 10]], device=DEV),
         'len_a': torch.tensor([3, 2], device=DEV), 'len_b': torch.tensor([2, 3], device=DEV), 'in_len': torch.tensor([T, T - 1], device=DEV),
         'lam': torch.tensor([0.3], device=DEV), 'lengths': torch.tensor([T, T - 2], dtype=torch.int32, device=DEV),
         'ys_out': torch.randint(1, V, (B * N, T // N), generator=g).to(DEV),
         'n_rows': torch.tensor([3, 2, 3, 3], dtype=torch.int32, device=DEV),
         'errors': torch.tensor([[0, 2], [1, 3]], dtype=torch.int32, device=DEV)}
    return d


def _loss(name, logits, d):
    """logits: [B, T, V], a view of the [R, 40] base"""
    from opentransformer_amd import ops
    V = logits.shape[-1]
    if name == 'ls':
        return ops.LabelSmoothingLossFn.apply(logits, d['target'], 0.1, 0)
    if name == 'ls_fused':
        return ops.label_smoothing_loss(logits, d['target'], 0.1, 0)
    if name == 'ctc':
        return ops.CTCLossFn.apply(logits, d['labels_a'], d['in_len'], d['len_a'], 0)
    if name == 'ctc_pair':
        return ops.ctc_loss_pair(logits, d['labels_a'], d['labels_b'], d['in_len'], d['len_a'], d['len_b'], d['lam'])[0]
    if name == 'mwer':
        return ops.mwer_loss(logits.view(B * N, T // N, V), d['ys_out'], d['n_rows'], d['errors'])[0]
    if name == 'distill':
        return ops.distill_loss(logits, d['teacher'], d['lengths'], temperature=2.0)[0]
    top_val, top_idx = ops.topk_rows(d['teacher'], d['lengths'], K)
    return ops.distill_loss_topk(logits, top_val, top_idx, d['lengths'], temperature=2.0)[0]


FN_OF = {'ls': 'LabelSmoothingLossFn', 'ls_fused': 'LabelSmoothingLossFusedFn', 'ctc': 'CTCLossFn', 'ctc_pair': 'CTCLossPairFn',
         'mwer': 'MwerLossFn', 'distill': 'DistillLossFn', 'distill_topk': 'DistillLossFn'}


def _grad(name, V, unit):
    """(the gradient of the [R, 40] base, what the Function handed to autograd: its zero-tail mark and the buffer behind it, a copy of
    the [R, ldd] buffer the forward saved)"""
    from opentransformer_amd import ops
    d = _data(V)
    base = d['buf'].clone().requires_grad_(True)
    logits = base[:, :V].view(B, T, V)
    handed = []
    logits.register_hook(lambda g: handed.append((ops._zero_tail_of(g), g._base if g._base is not None else g)))
    loss = _loss(name, logits, d)
    assert loss.grad_fn.name() == FN_OF[name] + 'Backward', loss.grad_fn.name()
    saved = loss.grad_fn.saved_tensors[0].clone().reshape(R, -1)
    if unit:
        ops.backward(loss)
    else:
        (2.5 * loss).backward()
    torch.cuda.synchronize()
    assert len(handed) == 1
    return base.grad, handed[0], saved


@pytest.mark.parametrize('V', WIDTHS)
@pytest.mark.parametrize('name', sorted(FN_OF))
def test_unit_seed_against_a_seed_of_2p5(name, V):
    g1, (tail1, root1), saved1 = _grad(name, V, unit=True)
    g2, (tail2, root2), saved2 = _grad(name, V, unit=False)
    assert float(g1.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    for seed, g, saved in ((1.0, g1, saved1), (2.5, g2, saved2)):           # each run against the buffer its own forward saved
        want = torch.zeros_like(g)
        want[:, :V] = seed * saved[:, :V]
        assert torch.equal(g, want), seed
    if name in FREE_ORDER:
        assert torch.equal(g2[:, 1:], 2.5 * g1[:, 1:])                      # across the runs: every column but the blank's
    else:
        assert torch.equal(saved1, saved2) and torch.equal(g2, 2.5 * g1)
    for g, tail, root in ((g1, tail1, root1), (g2, tail2, root2)):
        if V < LD:
            assert float(g[:, V:].abs().max()) == 0.0                       # the base buffer's gradient behind column V
        if V < LD and name in PADDED:                                       # what LinearFn.backward would read at its full width
            assert tail == (R, LD) and tuple(root.shape) == (R, LD) and float(root[:, V:].abs().max()) == 0.0
        else:
            assert tail is None and root.shape[-1] == V


@pytest.mark.parametrize('V', WIDTHS)
def test_the_switch_selects_the_label_smoothing_form(V):
    """tests/test_gpu_round5.py compares the two forms; with a dead switch it would compare one form with itself"""
    from opentransformer_amd import ops
    d = _data(V)
    logits = d['buf'].clone().requires_grad_(True)[:, :V].view(B, T, V)
    scale = torch.tensor([1024.0], device=DEV)

    def name(gs):
        loss = ops.label_smoothing_loss(logits, d['target'], 0.1, 0, grad_scale=gs)      # kept alive: its node dies with it
        return loss.grad_fn.name()
    was = ops._LS_FUSED
    assert was is True
    try:
        assert 'LabelSmoothingLossFusedFn' in name(None) and 'LabelSmoothingLossFusedFn' in name(scale)
        ops._LS_FUSED = False
        assert name(None) == 'LabelSmoothingLossFnBackward'
        assert name(scale) == 'ScaleGradFnBackward'
    finally:
        ops._LS_FUSED = was
