"""The loss wrappers over the C ABI (include/otrans_hip.h): label smoothing in its three-kernel and one-launch forms, CTC and its
MixSpeech pair form, MWER (of the attention model and of the CTC model), the transducer (joint, loss, greedy loop), distillation (dense and top-K) and topk_rows.  The rules are those of ops.py.  ops.py re-exports every
public name below; callers write `ops.X`.

Unlike decode_ops.py and data_ops.py this is no leaf: the losses need the autograd core (ScaleGradFn, the parked 16-bit hand-over,
the compute mode), which they reach at call time as `_ops.X`.  So this module is not to be imported before `ops`: the package
always imports `ops` first, and `ops.py` ends by importing this one.  The switch `_LS_FUSED` is owned by `ops`
(`ops._LS_FUSED`, OTR_SWITCHES=ops._LS_FUSED=0) and read there on every call; there is no copy of it here."""
import ctypes as C

import torch

from . import ops as _ops
from . import _lib as L
from ._runtime import _state, _cuda, _p, _stream, _timed, _len32
from .data_ops import _lam_check
from .decode_ops import log_softmax

__all__ = ['LabelSmoothingLossFn', 'LabelSmoothingLossFusedFn', 'label_smoothing_loss', 'CTCLossFn', 'CTC_MAX_TGT', 'CTCLossPairFn',
           'ctc_loss_pair', 'MWER_MAX_NBEST', 'MWER_MAX_V', 'MwerLossFn', 'mwer_loss', 'DISTILL_MAX_V', 'DISTILL_MAX_K', 'DistillLossFn',
           'distill_loss', 'distill_loss_topk', 'topk_rows']


# ---------------------------------------------------------------------------------------- what the losses share
def _f32(dev):
    """the allocator of a forward's fp32 outputs: f32(*shape)"""
    return lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)


def _rows_in_place(t, V):
    """(t2 [R, V], ld): the rows of t [..., V] as the kernels read them.  The head of a row-padded product (ops.padded_rows: rows of
    V8 = ceil8(V) floats), or any view with unit inner stride and a row stride >= V, is read in place; anything else is copied."""
    t2 = t.reshape(-1, V)
    if not (t2.stride(1) == 1 and (t2.shape[0] <= 1 or t2.stride(0) >= V)):
        t2 = t2.contiguous()
    return t2, (t2.stride(0) if t2.shape[0] > 1 else V)


def _grad_width(ld, V):
    """the row width of the gradient buffer: the padded width goes back to LinearFn.backward with a zero tail"""
    return ld if (V < ld < V + 8 and ld % 8 == 0) else V


def _unit_seed(g):
    """is g the cached unit seed of ops.backward?"""
    seed = _state.get(('unit_grad', g.device, g.dtype))
    return seed is not None and g.data_ptr() == seed.data_ptr()


def _saved_logits_grad(ctx, g, dlogits=None, alias_unit=True):
    """backward of a loss whose forward launch wrote d loss / d logits into a saved [..., ldd] buffer (every Function below; ctx.shape
    and ctx.V are the logits' shape and width): the buffer itself when g is the cached unit seed of ops.backward and alias_unit, else
    g times it; at a padded width it leaves as the head of a zero-tailed buffer.  dlogits: the buffer, where it is not the saved one."""
    if dlogits is None:
        (dlogits,) = ctx.saved_tensors
    if alias_unit and _unit_seed(g):
        out = dlogits                                              # g == 1: the saved buffer IS the gradient
    else:
        out = torch.empty_like(dlogits)
        g = g.contiguous().float()
        L.check(L.load().otr_scale(_p(dlogits), _p(out), dlogits.numel(), _p(g), 1.0, _stream()), 'otr_scale')
    if out.shape[-1] != ctx.V:
        out._otr_zero_tail = tuple(out.shape)                      # LinearFn.backward may read it at its full width (_zero_tail_of)
        out = out[:, :ctx.V]
    return out.view(ctx.shape)


# ---------------------------------------------------------------------------------------- label smoothing
class LabelSmoothingLossFn(torch.autograd.Function):
    """LabelSmoothingLoss.forward (module/loss.py:21-48) + its gradient in the same pass."""

    @staticmethod
    def forward(ctx, logits, target, smoothing, pad_idx):
        _cuda(logits, target)
        V = logits.shape[-1]
        lg = logits.reshape(-1, V)
        # the head of a row-padded product (ops.padded_rows: rows of V8 = ceil8(V) floats) is read in place, and the gradient
        # leaves as the head of a zero-tailed [R, V8] buffer.  Not _rows_in_place: this kernel takes one width for the logits and
        # the gradient, so only a padded, 16-byte aligned fp32 view stays in place and every other view is copied
        ld = lg.stride(0) if (lg.dim() == 2 and lg.shape[0] > 1 and lg.stride(1) == 1 and lg.dtype == torch.float32) else V
        if not (V < ld < V + 8 and ld % 8 == 0 and lg.data_ptr() % 16 == 0):
            lg, ld = lg.contiguous(), V
        R = lg.shape[0]
        tg = target.reshape(-1).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        dlogits = torch.empty((R, ld), dtype=torch.float32, device=lg.device) if ctx.needs_input_grad[0] else None
        scratch = torch.empty((R + 2,), dtype=torch.float32, device=lg.device)
        L.check(L.load().otr_label_smoothing_loss_ld(_p(lg), ld, _p(tg), R, V, smoothing, pad_idx, _p(loss), _p(dlogits), ld,
                                                     _p(scratch), _stream()), 'otr_label_smoothing_loss_ld')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        return loss

    @staticmethod
    def backward(ctx, g):
        # alias_unit=False: the unit seed is scaled into a fresh buffer too, as it always was; dropping that launch is its own change
        return _saved_logits_grad(ctx, g, alias_unit=False), None, None, None


class LabelSmoothingLossFusedFn(torch.autograd.Function):
    """LabelSmoothingLoss.forward + its gradient + the scalar factor of the backward seed in ONE launch (otr_label_smoothing_loss_fused).
    Semantics: loss = LabelSmoothingLossFn(...), d loss / d logits multiplied by `gscale` (a device scalar; None = 1) -- i.e.
    ScaleGradFn o LabelSmoothingLossFn.  The kernel writes gscale x d loss / d logits; backward multiplies by the incoming gradient,
    unless that is the cached unit seed of ops.backward (then the buffer leaves as it is: no launch)."""

    @staticmethod
    def forward(ctx, logits, ld, target, ldt, Lt, V, smoothing, pad_idx, gscale, ticket):
        lg = logits.reshape(-1, V)              # a view (label_smoothing_loss checked the strides)
        R = lg.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        need = ctx.needs_input_grad[0]
        # the logits' producer takes its output gradient as a 16-bit operand (_Grad16Link: the row-padded output layer): the
        # gradient is written in that type, one rounding where every other branch gradient of the model already has one
        g16 = getattr(logits, '_otr_g16', None)
        ctx.g16 = g16 if (need and g16 is not None and g16.armed and _ops.is_half() and ld % 8 == 0) else None
        ddt = _ops.half_dtype() if ctx.g16 is not None else torch.float32
        dlogits = torch.empty((R, ld), dtype=ddt, device=lg.device) if need else None
        scratch = torch.empty((R + 2,), dtype=torch.float32, device=lg.device)
        L.check(L.load().otr_label_smoothing_loss_fused(_p(lg), ld, _p(target), ldt, Lt, R, V, smoothing, pad_idx, _p(gscale), _p(loss),
                                                        _p(dlogits), _ops._code(ddt), ld, _p(scratch), _p(ticket), _stream()),
                'otr_label_smoothing_loss_fused')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        if ctx.g16 is not None:
            link = ctx.g16
            if _unit_seed(g) and link.buf is None and _ops._in_backward():
                link.buf = dlogits                                 # [R, ld] 16-bit, zero behind column V: LinearFn.backward's operand
                _ops._park(link)
                return (_ops._zero_placeholder(dlogits.device, ctx.shape),) + (None,) * 9
            dlogits = dlogits.float()                              # no hand-over: the general (fp32) route
        return (_saved_logits_grad(ctx, g, dlogits),) + (None,) * 9


def _ls_ticket(device):
    """the arrival counter of otr_label_smoothing_loss_fused: one zeroed uint32 per device, allocated outside any capture"""
    t = _state.setdefault('ls_ticket', {}).get(device)
    if t is None and not torch.cuda.is_current_stream_capturing():
        t = _state['ls_ticket'][device] = torch.zeros(4, dtype=torch.int32, device=device)
    return t


def label_smoothing_loss(logits, target, smoothing, pad_idx, grad_scale=None):
    """LabelSmoothingLoss (module/loss.py:21-48) of logits [..., V] against target [...]; with grad_scale (a device scalar, the loss
    scale) the gradient that flows back into the logits carries that factor (= ops.ScaleGradFn applied to the loss).  One launch where
    the fused kernel's alignment rules hold (fp32 logits with 16-byte aligned rows -- the row-padded output layer's are -- V <= 8192,
    <= 8192 rows), the three-kernel form + ScaleGradFn otherwise."""
    V = logits.shape[-1]
    lg = logits.reshape(-1, V)
    # the fused kernel's own gate, not _rows_in_place: it never copies, a view it cannot read in place takes the three-kernel form
    ok = (_ops._LS_FUSED and lg.is_cuda and lg.dtype == torch.float32 and lg.dim() == 2 and lg.stride(1) == 1 and V <= 8192
          and 0 < lg.shape[0] <= 8192 and lg.data_ptr() % 16 == 0 and target.dtype == torch.int64)
    if ok:
        ld = lg.stride(0) if lg.shape[0] > 1 else (V + 3) // 4 * 4
        ok = ld % 4 == 0 and V <= ld < V + 8
    ticket = _ls_ticket(lg.device) if ok else None
    if ok and ticket is not None:
        if target.dim() == 2 and target.stride(1) == 1 and target.stride(0) >= target.shape[1] and target.numel() == lg.shape[0]:
            tg, ldt, Lt = target, target.stride(0), target.shape[1]
        else:
            tg = target.reshape(-1).contiguous()
            ldt = Lt = tg.numel()
        if Lt <= 0x7fffffff and tg.numel() == lg.shape[0] and (lg.shape[0] == 1 or lg.shape[0] % Lt == 0):
            return LabelSmoothingLossFusedFn.apply(logits, ld, tg, ldt, Lt, V, smoothing, pad_idx, grad_scale, ticket)
    loss = LabelSmoothingLossFn.apply(logits, target, smoothing, pad_idx)
    return _ops.ScaleGradFn.apply(loss, grad_scale) if (grad_scale is not None and loss.requires_grad) else loss


# ---------------------------------------------------------------------------------------- CTC (csrc/ctc.hip)
class CTCLossFn(torch.autograd.Function):
    """CTCAssistor.compute_loss (model/ctc.py:50-53): log_softmax + CTC ('mean', zero_infinity)."""

    @staticmethod
    def forward(ctx, logits, targets, in_len, tgt_len, blank):
        _cuda(logits, targets, in_len, tgt_len)
        B, T, V = logits.shape
        lp = log_softmax(logits)
        tg = targets.contiguous()
        il, tl = _len32(in_len), _len32(tgt_len)
        max_tgt = tg.shape[1]
        f32 = _f32(logits.device)
        ws, nll, loss = f32(B, T, 2 * max_tgt + 1), f32(B), f32()
        dlogits = torch.empty_like(lp) if ctx.needs_input_grad[0] else None
        L.check(L.load().otr_ctc_loss(_p(lp), _p(tg), tg.stride(0), _p(il), _p(tl), B, T, V, max_tgt, blank, _p(ws),
                                      _p(nll), _p(loss), _p(dlogits), _stream()), 'otr_ctc_loss')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        return loss

    @staticmethod
    def backward(ctx, g):
        # alias_unit=False: the unit seed is scaled into a fresh buffer too, as it always was; dropping that launch is its own change
        return _saved_logits_grad(ctx, g, alias_unit=False), None, None, None, None


# ------------------------------------------------------------------ MixSpeech (csrc/mixspeech.hip, csrc/ctc.hip)
CTC_MAX_TGT = 127


class CTCLossPairFn(torch.autograd.Function):
    """The CTC term of MixSpeech (include/otrans_hip.h otr_ctc_loss_pair): ONE log-softmax of the logits, scored against two label sets
    with the device weights lam and 1 - lam, and one gradient lam * g_a + (1 - lam) * g_b written by the forward call.  Returns
    (loss, loss_a, loss_b, nll [2, P]); only loss is differentiable.  backward scales the saved gradient by the incoming seed
    (_saved_logits_grad: the buffer itself for the cached unit seed of ops.backward)."""

    @staticmethod
    def forward(ctx, logits, targets_a, targets_b, in_len, tgt_len_a, tgt_len_b, lam, blank):
        P, T, V = logits.shape
        lp = log_softmax(logits)
        max_tgt = targets_a.shape[1]
        f32 = _f32(logits.device)
        ws, nll, loss3 = f32(2, P, T, 2 * max_tgt + 1), f32(2, P), f32(3)
        dlogits = f32(P * T, V) if ctx.needs_input_grad[0] else None
        L.check(L.load().otr_ctc_loss_pair(_p(lp), _p(targets_a), targets_a.stride(0), _p(tgt_len_a), _p(targets_b), targets_b.stride(0),
                                           _p(tgt_len_b), _p(in_len), _p(lam), P, T, V, max_tgt, blank, _p(ws), _p(nll), _p(loss3),
                                           _p(dlogits), _stream()), 'otr_ctc_loss_pair')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        loss, loss_a, loss_b = loss3[0], loss3[1], loss3[2]
        ctx.mark_non_differentiable(loss_a, loss_b, nll)
        return loss, loss_a, loss_b, nll

    @staticmethod
    def backward(ctx, g, *_):
        return _saved_logits_grad(ctx, g), None, None, None, None, None, None, None


def _label_rows(who, name, t, P):
    if t.dim() != 2 or t.shape[0] != P:
        raise ValueError('%s: %s must be [P, W] = [%d, W], got %s' % (who, name, P, tuple(t.shape)))


def ctc_loss_pair(logits, targets_a, targets_b, in_len, tgt_len_a, tgt_len_b, lam, blank=0):
    """lam * CTC(logits, a) + (1 - lam) * CTC(logits, b) in one call (include/otrans_hip.h otr_ctc_loss_pair), each term what CTCLossFn
    computes for that label set alone ('mean' over the P utterances of nll / max(L, 1), zero_infinity).  logits f32 [P, T, V];
    targets_a / targets_b int64 [P, W], W <= 127, unit inner stride -- views with a longer row stride (the even and odd rows of one
    matrix) are read in place; in_len, tgt_len_a, tgt_len_b [P] (int32 or int64); lam a 1-element f32 DEVICE tensor, never read by the
    host.  Returns (loss, loss_a, loss_b): loss carries the gradient, loss_a and loss_b are detached device scalars.  One log-softmax,
    three launches, no host synchronisation: capturable."""
    who = 'ctc_loss_pair'
    if logits.dim() != 3:
        raise ValueError('%s: logits must be [P, T, V], got %s' % (who, tuple(logits.shape)))
    P, T, V = logits.shape
    if P < 1 or T < 1 or V < 2:
        raise ValueError('%s: logits [P, T, V] = %s need P >= 1, T >= 1 and V >= 2' % (who, (P, T, V)))
    _label_rows(who, 'targets_a', targets_a, P)
    _label_rows(who, 'targets_b', targets_b, P)
    if targets_a.shape[1] != targets_b.shape[1]:
        raise ValueError('%s: the two label sets have widths %d and %d, one padded width expected' % (who, targets_a.shape[1], targets_b.shape[1]))
    if targets_a.shape[1] > CTC_MAX_TGT:
        raise ValueError('%s: target width %d > %d not supported' % (who, targets_a.shape[1], CTC_MAX_TGT))
    for name, t in (('in_len', in_len), ('tgt_len_a', tgt_len_a), ('tgt_len_b', tgt_len_b)):
        if t.numel() != P:
            raise ValueError('%s: %s must hold P = %d entries, got %s' % (who, name, P, tuple(t.shape)))
    _lam_check(who, lam)
    if not 0 <= int(blank) < V:
        raise ValueError('%s: blank=%r outside [0, V=%d)' % (who, blank, V))
    _cuda(logits, targets_a, targets_b, in_len, tgt_len_a, tgt_len_b, lam)
    if (logits.dtype != torch.float32 or targets_a.dtype != torch.int64 or targets_b.dtype != torch.int64 or lam.dtype != torch.float32
            or any(t.dtype not in (torch.int32, torch.int64) for t in (in_len, tgt_len_a, tgt_len_b))):
        raise L.OtransHipError('%s: logits f32, targets int64, lengths int32 (or int64), lam f32 expected' % who)
    W = targets_a.shape[1]
    rows = [t if (t.stride(1) == 1 and t.stride(0) >= W) or W == 0 else t.contiguous() for t in (targets_a, targets_b)]
    lens = [_len32(t) for t in (in_len, tgt_len_a, tgt_len_b)]
    loss, loss_a, loss_b, _ = CTCLossPairFn.apply(logits, rows[0], rows[1], lens[0], lens[1], lens[2], lam.detach(), int(blank))
    return loss, loss_a, loss_b


# ------------------------------------------------------------------ minimum word error rate training (csrc/mwer.hip)
MWER_MAX_NBEST, MWER_MAX_V = 32, 8192


class MwerLossFn(torch.autograd.Function):
    """The N-best expected number of errors (include/otrans_hip.h otr_mwer_loss) of teacher-forced logits [B*N*max_len, V] (any leading
    shape) + its gradient in the same call when the logits need one, like LabelSmoothingLossFn.  The head of a row-padded product
    (ops.padded_rows: rows of V8 = ceil8(V) floats) is read in place and the gradient leaves as the head of a zero-tailed [R, V8]
    buffer.  `gscale` (a device scalar; None = 1) rides in the written gradient; backward multiplies by the incoming gradient unless
    that is the cached unit seed of ops.backward.  Returns (loss, seq_logp [B*N], post [B, N], utt_err [B]); only loss is
    differentiable.  The gradient is fp32: a 16-bit hand-over armed by the logits' Linear (_Grad16Link) is left unused."""

    @staticmethod
    def forward(ctx, logits, ys_out, n_rows, errors, gscale):
        V = logits.shape[-1]
        B, N = errors.shape
        max_len = ys_out.shape[1]
        lg, ld = _rows_in_place(logits, V)
        R, ldd = lg.shape[0], _grad_width(ld, V)
        f32 = _f32(lg.device)
        loss, seq_logp, post, utt_err = f32(), f32(B * N), f32(B, N), f32(B)
        dlogits = f32(R, ldd) if ctx.needs_input_grad[0] else None
        lib = L.load()
        nws = lib.otr_mwer_workspace_floats(B, N, max_len)
        ws = f32(max(nws, 1))
        L.check(_timed('mwer_loss %dx%dx%dx%d' % (B, N, max_len, V), {'bytes': R * (2 * V + ldd) * 4},
                       lambda: lib.otr_mwer_loss(_p(lg), ld, _p(ys_out), ys_out.stride(0), _p(n_rows), _p(errors), B, N, max_len, V,
                                                 _p(gscale), _p(loss), _p(seq_logp), _p(post), _p(utt_err), _p(dlogits), ldd, _p(ws),
                                                 ws.numel(), _stream())), 'otr_mwer_loss')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        ctx.mark_non_differentiable(seq_logp, post, utt_err)
        return loss, seq_logp, post, utt_err

    @staticmethod
    def backward(ctx, g, *_):
        return _saved_logits_grad(ctx, g), None, None, None, None


def mwer_loss(logits, ys_out, n_rows, errors, grad_scale=None):
    """Minimum word error rate loss over an n-best list (include/otrans_hip.h otr_mwer_loss).  logits f32 [B*N, max_len, >= V] or
    [B*N*max_len, V] with unit stride along the vocabulary (a view with a longer row stride is read in place): the teacher-forced
    decoder output on rescore_pack's ys_in; ys_out int64 [B*N, max_len] and n_rows int32 [B*N] from rescore_pack; errors int32 [B, N]
    from edit_distance (< 0: the slot is left out).  grad_scale: a device scalar the gradient into the logits is multiplied by (the
    loss scale), None = 1.  Returns (loss, {'seq_logp' [B, N] (-inf: not live), 'post' [B, N], 'utt_err' [B]}), the dict detached.
    At most three launches on the current stream, no host synchronisation, the same bits on every run: capturable."""
    if errors.dim() != 2 or ys_out.dim() != 2 or ys_out.shape[0] != errors.numel() or n_rows.numel() != errors.numel():
        raise ValueError('mwer_loss: errors must be [B, N], ys_out [B*N, max_len] and n_rows [B*N], got %s, %s and %s'
                         % (tuple(errors.shape), tuple(ys_out.shape), tuple(n_rows.shape)))
    B, N = errors.shape
    V, max_len = logits.shape[-1], ys_out.shape[1]
    if not 1 <= N <= MWER_MAX_NBEST:
        raise ValueError('mwer_loss: N=%d hypotheses per utterance must be in [1, %d]' % (N, MWER_MAX_NBEST))
    if not 1 <= V <= MWER_MAX_V:
        raise ValueError('mwer_loss: vocabulary V=%d must be in [1, %d]' % (V, MWER_MAX_V))
    if max_len < 1 or B * N * max_len >= 1 << 30:
        raise ValueError('mwer_loss: B*N*max_len = %d*%d*%d must be in [1, 2^30)' % (B, N, max_len))
    if logits.numel() != B * N * max_len * V:
        raise ValueError('mwer_loss: logits %s do not hold B*N*max_len = %d rows of V = %d' % (tuple(logits.shape), B * N * max_len, V))
    _cuda(logits, ys_out, n_rows, errors, grad_scale)
    if (logits.dtype != torch.float32 or ys_out.dtype != torch.int64 or n_rows.dtype != torch.int32 or errors.dtype != torch.int32
            or ys_out.stride(1) != 1 or ys_out.stride(0) < max_len):
        raise L.OtransHipError('mwer_loss: logits f32, ys_out int64 (rows contiguous), n_rows int32, errors int32 expected')
    loss, seq_logp, post, utt_err = MwerLossFn.apply(logits, ys_out, n_rows.contiguous(), errors.contiguous(), grad_scale)
    return loss, {'seq_logp': seq_logp.view(B, N), 'post': post, 'utt_err': utt_err}


# ------------------------------------------------------------------ MWER training of the CTC model (csrc/ctc.hip)
class CtcMwerLossFn(torch.autograd.Function):
    """The N-best expected number of errors of a CTC head (include/otrans_hip.h otr_ctc_mwer_loss), with the interpolated CTC loss on
    the reference where one is given: ONE log-softmax of the logits, scored against N hypotheses per utterance (+ the reference), and
    one gradient written by the forward call when the logits need one.  `gscale` (a device scalar; None = 1) rides in the written
    gradient.  Returns (loss, mwer, ctc, seq_logp [B, N], post [B, N], utt_err [B]); only loss is differentiable.  backward scales
    the saved gradient by the incoming seed (_saved_logits_grad: the buffer itself for the cached unit seed of ops.backward)."""

    @staticmethod
    def forward(ctx, logits, in_len, hyps, hyp_len, errors, ref, ref_len, ctc_weight, scale, blank, gscale, max_tgt):
        B, T, V = logits.shape
        N = errors.shape[1]
        lp = log_softmax(logits)
        f32 = _f32(logits.device)
        loss3, seq_logp, post, utt_err, nll_ref = f32(3), f32(B, N), f32(B, N), f32(B), f32(B)
        need = ctx.needs_input_grad[0]
        dlogits = f32(B * T, V) if need else None
        lib = L.load()
        ws = f32(max(lib.otr_ctc_mwer_workspace_floats(B, N, T, max_tgt), 1))
        L.check(_timed('ctc_mwer_loss %dx%dx%dx%d' % (B, N, T, V), {'bytes': B * T * (V * (2 if need else 1) + (N + 1) * (2 * max_tgt + 1)) * 4},
                       lambda: lib.otr_ctc_mwer_loss(_p(lp), _p(in_len), _p(hyps), hyps.stride(1), _p(hyp_len), _p(errors), _p(ref),
                                                     ref.stride(0) if ref is not None else 0, _p(ref_len), ctc_weight, scale, _p(gscale),
                                                     B, N, T, V, max_tgt, blank, _p(loss3), _p(seq_logp), _p(post), _p(utt_err),
                                                     _p(nll_ref), _p(dlogits), _p(ws), ws.numel(), _stream())), 'otr_ctc_mwer_loss')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        loss, mwer, ctc = loss3[0], loss3[1], loss3[2]
        ctx.mark_non_differentiable(mwer, ctc, seq_logp, post, utt_err)
        return loss, mwer, ctc, seq_logp, post, utt_err

    @staticmethod
    def backward(ctx, g, *_):
        return (_saved_logits_grad(ctx, g),) + (None,) * 11


def _label_width(t, width):
    """t [..., W] as the entry reads it: unit inner stride, at least `width` labels per row (padded with -1, which no length reaches:
    a label the kernel would refuse) and at most `width` of them looked at"""
    if t.shape[-1] < width:
        t = torch.nn.functional.pad(t, (0, width - t.shape[-1]), value=-1)
    return t if t.stride(-1) == 1 else t.contiguous()


def ctc_mwer_loss(logits, in_len, hyps, hyp_len, errors, ref=None, ref_len=None, ctc_weight=0.0, scale=1.0, blank=0, grad_scale=None):
    """Minimum word error rate loss of a CTC head over an n-best list, mwer + ctc_weight * CTC(ref), in one call (include/otrans_hip.h
    otr_ctc_mwer_loss).  logits f32 [B, T, V] (the head's raw output: ONE log-softmax is taken here); in_len [B] frames per utterance;
    hyps int64 [B, N, L] tokens with unit stride along L (what ops.ctc_prefix_beam_search returns; a view whose rows are evenly strided
    is read in place), hyp_len [B, N], errors int32 [B, N] from ops.edit_distance (< 0: the slot is left out).  A slot also takes no
    part if its length is outside [0, min(L, 127)], a label inside its length is outside [0, V), or the labels do not fit into the
    frames; nothing behind a length is read.  ref int64 [B, W] (W <= 127) and ref_len [B]: the reference labels of the interpolated
    CTC term ('mean' over the B utterances of nll / max(L, 1), zero_infinity: what CTCLossFn computes), both or neither.  P_n =
    softmax_n(scale * ll_n) over the live slots.  grad_scale: a device scalar the gradient into the logits is multiplied by (the loss
    scale), None = 1.  Returns (loss, {'mwer', 'ctc' (scalars), 'seq_logp' [B, N] (-inf: not live), 'post' [B, N], 'utt_err' [B]}),
    the dict detached.  Four launches behind the log-softmax (two without a gradient), no host synchronisation: capturable.  The
    scalars and the dict have the same bits on every run; the gradient's occupancies are added with atomics, as CTCLossFn's."""
    who = 'ctc_mwer_loss'
    if logits.dim() != 3:
        raise ValueError('%s: logits must be [B, T, V], got %s' % (who, tuple(logits.shape)))
    B, T, V = logits.shape
    if not 1 <= B <= 65535 or T < 1 or V < 2:
        raise ValueError('%s: logits [B, T, V] = %s need 1 <= B <= 65535, T >= 1 and V >= 2' % (who, (B, T, V)))
    if hyps.dim() != 3 or hyps.shape[0] != B or errors.dim() != 2 or tuple(errors.shape) != tuple(hyps.shape[:2]) or hyp_len.numel() != errors.numel():
        raise ValueError('%s: hyps must be [B, N, L] = [%d, N, L], hyp_len and errors [B, N], got %s, %s and %s'
                         % (who, B, tuple(hyps.shape), tuple(hyp_len.shape), tuple(errors.shape)))
    N, Lh = hyps.shape[1], hyps.shape[2]
    if not 1 <= N <= MWER_MAX_NBEST:
        raise ValueError('%s: N=%d hypotheses per utterance must be in [1, %d]' % (who, N, MWER_MAX_NBEST))
    if in_len.numel() != B:
        raise ValueError('%s: in_len must hold B = %d entries, got %s' % (who, B, tuple(in_len.shape)))
    if (ref is None) != (ref_len is None):
        raise ValueError('%s: ref and ref_len go together (both or neither)' % who)
    if ref is not None:
        _label_rows(who, 'ref', ref, B)
        if ref.shape[1] > CTC_MAX_TGT:
            raise ValueError('%s: reference width %d > %d not supported' % (who, ref.shape[1], CTC_MAX_TGT))
        if ref_len.numel() != B:
            raise ValueError('%s: ref_len must hold B = %d entries, got %s' % (who, B, tuple(ref_len.shape)))
    ctc_weight, scale = float(ctc_weight), float(scale)
    if not 0 <= ctc_weight < float('inf'):
        raise ValueError('%s: ctc_weight=%r must be finite and >= 0' % (who, ctc_weight))
    if not 0 < scale < float('inf'):
        raise ValueError('%s: scale=%r must be finite and > 0' % (who, scale))
    if not 0 <= int(blank) < V:
        raise ValueError('%s: blank=%r outside [0, V=%d)' % (who, blank, V))
    _cuda(logits, in_len, hyps, hyp_len, errors, ref, ref_len, grad_scale)
    if (logits.dtype != torch.float32 or hyps.dtype != torch.int64 or errors.dtype != torch.int32 or (ref is not None and ref.dtype != torch.int64)
            or any(t is not None and t.dtype not in (torch.int32, torch.int64) for t in (in_len, hyp_len, ref_len))
            or (grad_scale is not None and grad_scale.dtype != torch.float32)):
        raise L.OtransHipError('%s: logits f32, hyps and ref int64, errors int32, lengths int32 (or int64), grad_scale f32 expected' % who)
    # one bound for both label sets.  L is narrowed to 127 whatever the lengths are: a hypothesis longer than that is left to the kernel,
    # which counts its slot as dead (no host read of hyp_len)
    max_tgt = min(max(Lh, ref.shape[1] if ref is not None else 0), CTC_MAX_TGT)
    hyps = _label_width(hyps, max(max_tgt, 1))
    if hyps.stride(0) != N * hyps.stride(1) or hyps.stride(1) < max_tgt:       # row (b, n) is read at (b * N + n) * stride(1)
        hyps = hyps.contiguous()
    if ref is not None:
        ref = _label_width(ref, max(max_tgt, 1))
        if ref.stride(0) < max_tgt:
            ref = ref.contiguous()
    out = CtcMwerLossFn.apply(logits, _len32(in_len), hyps, _len32(hyp_len), errors.contiguous(), ref,
                              _len32(ref_len) if ref_len is not None else None, ctc_weight, scale, int(blank), grad_scale, max_tgt)
    loss, mwer, ctc, seq_logp, post, utt_err = out
    return loss, {'mwer': mwer, 'ctc': ctc, 'seq_logp': seq_logp, 'post': post, 'utt_err': utt_err}


# ------------------------------------------------------------------ the transducer (csrc/rnnt.hip)
RNNT_MAX_TGT = 255          # include/otrans_hip.h OTR_RNNT_MAX_TGT: at most 256 lattice columns


def _rnnt_int_vector(who, name, t, B):
    if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64):
        raise ValueError('%s: %s must be an int32 or int64 tensor, got %s' % (who, name, getattr(t, 'dtype', type(t).__name__)))
    if t.numel() != B:
        raise ValueError('%s: %s must hold B = %d entries, got %s' % (who, name, B, tuple(t.shape)))


class RnntLossFn(torch.autograd.Function):
    """The transducer loss (include/otrans_hip.h otr_rnnt_loss) of the joint's RAW logits [B, T, U1, V]: one log-softmax, the alpha and
    beta sweeps and, when the logits need one, the gradient, all written by the forward call.  The head of a row-padded product is
    read in place and the gradient leaves as the head of a zero-tailed buffer, as in MwerLossFn.  `gscale` (a device scalar; None = 1)
    rides in the written gradient.  Returns (loss, nll [B], valid int32 [B]); only loss is differentiable.  backward scales the saved
    gradient by the incoming seed (_saved_logits_grad: the buffer itself for the cached unit seed of ops.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, enc_len, tgt_len, blank, gscale):
        B, T, U1, V = logits.shape
        lg, ld = _rows_in_place(logits, V)
        R, ldd = lg.shape[0], _grad_width(ld, V)
        f32 = _f32(lg.device)
        loss, nll = f32(), f32(B)
        valid = torch.empty((B,), dtype=torch.int32, device=lg.device)
        need = ctx.needs_input_grad[0]
        dlogits = f32(R, ldd) if need else None
        lib = L.load()
        ws = f32(max(lib.otr_rnnt_workspace_floats(B, T, U1), 1))
        L.check(_timed('rnnt_loss %dx%dx%dx%d' % (B, T, U1, V), {'bytes': R * (V + (V + ldd if need else 0)) * 4},
                       lambda: lib.otr_rnnt_loss(_p(lg), ld, _p(labels), labels.stride(0) if U1 > 1 else 0, _p(enc_len), _p(tgt_len), B, T, U1,
                                                 V, blank, _p(gscale), _p(loss), _p(nll), _p(valid), _p(dlogits), ldd, _p(ws), ws.numel(),
                                                 _stream())), 'otr_rnnt_loss')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = logits.shape, V
        ctx.mark_non_differentiable(nll, valid)
        return loss, nll, valid

    @staticmethod
    def backward(ctx, g, *_):
        return _saved_logits_grad(ctx, g), None, None, None, None, None


def rnnt_loss(logits, enc_len, labels, tgt_len, blank=0, grad_scale=None):
    """The transducer (RNN-T) loss in one call (include/otrans_hip.h otr_rnnt_loss): (1 / B) sum_b -ln P(y_b | x_b) over the lattice of
    the joint's logits.  logits f32 [B, T, U + 1, V] RAW (one log-softmax is taken here), unit stride along V (the head of a row-padded
    product is read in place); enc_len [B] frames and tgt_len [B] labels per utterance (int32 or int64); labels int64 [B, >= U] with
    unit inner stride: y_1 .. y_U, a view such as truth[:, 1:-1] is read in place.  U + 1 <= RNNT_MAX_TGT + 1 = 256.  An utterance
    with a length out of range or a label outside [0, V) or equal to blank is guarded on the device: nll 0, valid 0, zero gradient,
    still counted in 1 / B.  grad_scale: a device scalar the gradient into the logits is multiplied by (the loss scale), None = 1.
    Returns (loss, {'nll' [B], 'valid' int32 [B]}), the dict detached.  Four launches (three without a gradient), no atomics, no host
    synchronisation: the same bits on every run, capturable."""
    who = 'rnnt_loss'
    if logits.dim() != 4:
        raise ValueError('%s: logits must be [B, T, U + 1, V], got %s' % (who, tuple(logits.shape)))
    B, T, U1, V = logits.shape
    if not 1 <= B <= 65535 or not 1 <= T <= 65535 or U1 < 1 or V < 2:
        raise ValueError('%s: logits [B, T, U + 1, V] = %s need 1 <= B, T <= 65535, U + 1 >= 1 and V >= 2' % (who, (B, T, U1, V)))
    if U1 > RNNT_MAX_TGT + 1:
        raise ValueError('%s: U + 1 = %d lattice columns > %d not supported' % (who, U1, RNNT_MAX_TGT + 1))
    if B * T * U1 >= (1 << 31) - 4:
        raise ValueError('%s: B*T*(U + 1) = %d*%d*%d rows must stay below 2^31' % (who, B, T, U1))
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] < U1 - 1:
        raise ValueError('%s: labels must be [B, >= U] = [%d, >= %d], got %s' % (who, B, U1 - 1, tuple(getattr(labels, 'shape', ()))))
    if labels.dtype != torch.int64:
        raise ValueError('%s: labels must be int64, got %s' % (who, labels.dtype))
    _rnnt_int_vector(who, 'enc_len', enc_len, B)
    _rnnt_int_vector(who, 'tgt_len', tgt_len, B)
    if not 0 <= int(blank) < V:
        raise ValueError('%s: blank=%r outside [0, V=%d)' % (who, blank, V))
    _cuda(logits, labels, enc_len, tgt_len, grad_scale)
    if logits.dtype != torch.float32 or (grad_scale is not None and grad_scale.dtype != torch.float32):
        raise L.OtransHipError('%s: logits f32 and grad_scale f32 expected' % who)
    if U1 > 1 and not (labels.stride(1) == 1 and labels.stride(0) >= U1 - 1):
        labels = labels.contiguous()
    loss, nll, valid = RnntLossFn.apply(logits, labels, _len32(enc_len), _len32(tgt_len), int(blank), grad_scale)
    return loss, {'nll': nll, 'valid': valid}


class RnntJointFn(torch.autograd.Function):
    """The transducer's joint activation z[b,t,u,:] = tanh(pe[b,t,:] + pg[b,u,:]) inside the lengths, zeros outside (include/otrans_hip.h
    otr_rnnt_joint_fwd) -> (z f32 [B, T, U1, J], its 16-bit twin or None).  Backward (otr_rnnt_joint_bwd): dpe = sum_u dz (1 - z^2),
    dpg = sum_t dz (1 - z^2), two launches that each read dz and z once; what lies outside the lengths is never read."""

    @staticmethod
    def forward(ctx, pe, pg, enc_len, tgt_len):
        B, T, J = pe.shape
        U1 = pg.shape[1]
        z = torch.empty((B, T, U1, J), dtype=torch.float32, device=pe.device)
        z16 = torch.empty((B, T, U1, J), dtype=_ops.half_dtype(), device=pe.device) if _ops.is_half() else None
        L.check(_timed('rnnt_joint_fwd %dx%dx%dx%d' % (B, T, U1, J), {'bytes': z.numel() * (6 if z16 is not None else 4)},
                       lambda: L.load().otr_rnnt_joint_fwd(_p(pe), _p(pg), _p(enc_len), _p(tgt_len), B, T, U1, J, _p(z), _p(z16), _stream())),
                'otr_rnnt_joint_fwd')
        ctx.save_for_backward(z, enc_len, tgt_len)
        if z16 is not None:
            ctx.mark_non_differentiable(z16)
        return z, z16

    @staticmethod
    def backward(ctx, dz, _dz16=None):
        z, enc_len, tgt_len = ctx.saved_tensors
        B, T, U1, J = z.shape
        dz = dz.contiguous().float()
        dpe = torch.empty((B, T, J), dtype=torch.float32, device=z.device)
        dpg = torch.empty((B, U1, J), dtype=torch.float32, device=z.device)
        L.check(_timed('rnnt_joint_bwd %dx%dx%dx%d' % (B, T, U1, J), {'bytes': z.numel() * 16},
                       lambda: L.load().otr_rnnt_joint_bwd(_p(dz), _p(z), _p(enc_len), _p(tgt_len), B, T, U1, J, _p(dpe), _p(dpg), _stream())),
                'otr_rnnt_joint_bwd')
        return dpe, dpg, None, None


def rnnt_joint(pe, pg, enc_len, tgt_len):
    """z = tanh(pe[:, :, None, :] + pg[:, None, :, :]) f32 [B, T, U + 1, J] with its 16-bit twin attached, zeros where t >= enc_len[b] or
    u > tgt_len[b]; pe f32 [B, T, J] (the encoder projection), pg f32 [B, U + 1, J] (the predictor projection), J a multiple of 4,
    U + 1 <= RNNT_MAX_TGT + 1.  Autograd to pe and pg."""
    who = 'rnnt_joint'
    if pe.dim() != 3 or pg.dim() != 3 or pe.shape[0] != pg.shape[0] or pe.shape[2] != pg.shape[2]:
        raise ValueError('%s: pe must be [B, T, J] and pg [B, U + 1, J], got %s and %s' % (who, tuple(pe.shape), tuple(pg.shape)))
    B, T, J = pe.shape
    U1 = pg.shape[1]
    if J < 4 or J % 4:
        raise ValueError('%s: J=%d must be a positive multiple of 4' % (who, J))
    if U1 > RNNT_MAX_TGT + 1:
        raise ValueError('%s: U + 1 = %d lattice columns > %d not supported' % (who, U1, RNNT_MAX_TGT + 1))
    if not 1 <= B <= 65535 or not 1 <= T <= 65535 or U1 < 1 or B * T * U1 >= (1 << 31) - 4:
        raise ValueError('%s: [B, T, U + 1] = %s need 1 <= B, T <= 65535, U + 1 >= 1 and B*T*(U + 1) < 2^31' % (who, (B, T, U1)))
    _rnnt_int_vector(who, 'enc_len', enc_len, B)
    _rnnt_int_vector(who, 'tgt_len', tgt_len, B)
    _cuda(pe, pg, enc_len, tgt_len)
    if pe.dtype != torch.float32 or pg.dtype != torch.float32:
        raise L.OtransHipError('%s: pe and pg must be f32, got %s and %s' % (who, pe.dtype, pg.dtype))
    z, z16 = RnntJointFn.apply(pe.contiguous(), pg.contiguous(), _len32(enc_len), _len32(tgt_len))
    return _ops.attach_lp(z, z16)


@torch.no_grad()
def rnnt_greedy(pe, enc_len, predictor_step, output, max_symbols=4, max_len=200, blank=0, bos=1):
    """Greedy transducer decoding of a batch, all state on the device.  pe f32 [B, T, J]: the joint's encoder projection; enc_len [B].
    predictor_step(tokens int64 [B, 1], h, c) -> (h', c', pg' f32 [B, J]): one predictor step for all rows from the per-layer state
    lists h / c (None: the zero state; every h carries its 16-bit twin in the 16-bit modes) to the new lists and the joint's predictor
    projection.  output(z) -> logits f32 [B, V].  Per step: otr_rnnt_greedy_joint, output, otr_rnnt_greedy_advance (arg-max; a row
    emits unless the arg-max is blank or max_symbols tokens were already emitted at its frame, else it moves to the next frame),
    predictor_step on the step's tokens, otr_rnnt_greedy_commit (the candidate state replaces the committed one where a row emitted).
    At most T + max_len steps; the count of unfinished rows is read on the host every 16th step.  Returns (tokens int64 [B, max_len],
    lengths int32 [B], scores f32 [B]: the sum of the log-probs of every decision, frames int32 [B, max_len]: the frame of each token)."""
    who = 'rnnt_greedy'
    if pe.dim() != 3:
        raise ValueError('%s: pe must be [B, T, J], got %s' % (who, tuple(pe.shape)))
    B, T, J = pe.shape
    if J < 4 or J % 4:
        raise ValueError('%s: J=%d must be a positive multiple of 4' % (who, J))
    if not 1 <= B <= 65535 or T < 1:
        raise ValueError('%s: pe [B, T, J] = %s needs 1 <= B <= 65535 and T >= 1' % (who, (B, T, J)))
    for name, v in (('max_symbols', max_symbols), ('max_len', max_len)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError('%s: %s=%r must be an integer >= 1' % (who, name, v))
    _rnnt_int_vector(who, 'enc_len', enc_len, B)
    _cuda(pe, enc_len)
    if pe.dtype != torch.float32:
        raise L.OtransHipError('%s: pe must be f32, got %s' % (who, pe.dtype))
    pe, dev, lib = pe.contiguous(), pe.device, L.load()
    half = _ops.is_half()
    el = _len32(enc_len)
    i32 = lambda *sh: torch.zeros(sh, dtype=torch.int32, device=dev)      # noqa: E731
    t, n, cnt, emit, frames = i32(B), i32(B), i32(B), i32(B), i32(B, max_len)
    tokens = torch.zeros((B, max_len), dtype=torch.int64, device=dev)
    score = torch.zeros((B,), dtype=torch.float32, device=dev)
    step_tok = torch.full((B,), int(bos), dtype=torch.int64, device=dev)
    remaining = (el.clamp(0, T) > 0).sum().to(torch.int32).view(1)
    h, c, pg = predictor_step(step_tok.view(B, 1), None, None)           # the committed state: the predictor after BOS
    pg = pg.contiguous()

    def items(hs, cs, g):
        out = list(hs) + list(cs) + [g]
        if half:
            out += [_ops.lp_of(x) for x in hs]
        return out
    dst = items(h, c, pg)
    if any(x is None or not x.is_contiguous() for x in dst):
        raise L.OtransHipError('%s: predictor_step must return contiguous states (with their 16-bit twins in the 16-bit modes)' % who)
    # the commit entry takes at most 16 items a call: 3 per layer + 1 in the 16-bit modes, so a deep predictor takes more than one call
    cuts = [(i, min(i + 16, len(dst))) for i in range(0, len(dst), 16)]
    nbytes = [(C.c_int32 * (j - i))(*[x.shape[-1] * x.element_size() for x in dst[i:j]]) for i, j in cuts]
    dst_p = [(C.c_void_p * (j - i))(*[x.data_ptr() for x in dst[i:j]]) for i, j in cuts]
    z = torch.empty((B, J), dtype=torch.float32, device=dev)
    z16 = torch.empty((B, J), dtype=_ops.half_dtype(), device=dev) if half else None
    st = _stream()
    for step in range(T + max_len):
        L.check(lib.otr_rnnt_greedy_joint(_p(pe), _p(pg), _p(t), _p(n), _p(el), B, T, J, max_len, _p(z), _p(z16), st), 'otr_rnnt_greedy_joint')
        logits = output(_ops.attach_lp(z, z16))
        V = logits.shape[-1]
        lg, ld = _rows_in_place(logits, V)
        L.check(lib.otr_rnnt_greedy_advance(_p(lg), ld, _p(el), B, T, V, int(blank), max_symbols, max_len, _p(t), _p(n), _p(cnt), _p(tokens),
                                            _p(frames), _p(score), _p(emit), _p(step_tok), _p(remaining), st), 'otr_rnnt_greedy_advance')
        h1, c1, pg1 = predictor_step(step_tok.view(B, 1), h, c)
        src = items(h1, c1, pg1.contiguous())
        for k, (i, j) in enumerate(cuts):
            src_p = (C.c_void_p * (j - i))(*[x.data_ptr() for x in src[i:j]])
            L.check(lib.otr_rnnt_greedy_commit(_p(emit), src_p, dst_p[k], nbytes[k], j - i, B, st), 'otr_rnnt_greedy_commit')
        if step % 16 == 15 and int(remaining) == 0:
            break
    return tokens, n, score, frames


# ------------------------------------------------------------------ the transducer's beam search (csrc/rnntbeam.hip)
RNNT_BEAM_MAX, RNNT_BEAM_MAX_LEN = 16, 256      # include/otrans_hip.h OTR_RNNT_BEAM_MAX, OTR_RNNT_BEAM_MAX_LEN


def rnnt_beam_limits(who, beam_width, max_len):
    """the limits of the search that need no tensor (TransducerRecognizer checks them in its constructor too)"""
    for name, v in (('beam_width', beam_width), ('max_len', max_len)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError('%s: %s=%r must be an integer' % (who, name, v))
    if not 1 <= beam_width <= RNNT_BEAM_MAX:
        raise ValueError('%s: beam_width=%d must be in [1, %d]' % (who, beam_width, RNNT_BEAM_MAX))
    if not 1 <= max_len <= RNNT_BEAM_MAX_LEN:
        raise ValueError('%s: max_len=%d must be in [1, %d]' % (who, max_len, RNNT_BEAM_MAX_LEN))


@torch.no_grad()
def rnnt_beam(pe, enc_len, predictor_step, output, beam_width=4, max_len=200, blank=0, bos=1):
    """Beam search of the transducer, all state on the device: frame-synchronous, at most ONE symbol per frame, hypotheses that name the
    same token sequence merged (logaddexp) before pruning -- "modified beam search"; include/otrans_hip.h (otr_rnnt_beam_select)
    states a frame in full.  pe f32 [B, T, J]: the joint's encoder projection; enc_len [B].  predictor_step and output are
    rnnt_greedy's callbacks, here on B * W rows (slot r belongs to utterance r // W); the first predictor_step runs on B rows of
    `bos` and its result is placed in slot 0 of every utterance.  Per frame: otr_rnnt_beam_joint, output, otr_rnnt_beam_select,
    otr_rnnt_beam_gather (the committed predictor state follows its hypothesis to the new slot, into the other half of a double
    buffer), predictor_step on the step's tokens, otr_rnnt_greedy_commit (the candidate state replaces the committed one where the slot
    was extended).  Exactly T iterations; nothing is read back on the way.  Returns (tokens int64 [B, W, max_len], lengths int32
    [B, W], scores f32 [B, W], frames int32 [B, W, max_len]: the frame of each token), best first; a slot that never became live has
    score -inf and length 0, and everything behind a length is 0.
    The score is the log of the summed probability of the alignments the search kept.  It is NOT rnnt_greedy's score: greedy pays a
    blank to leave a frame after an emission, this search moves to the next frame with every candidate, stay or extension.  For
    the same reason beam_width=1 -- one-symbol-per-frame arg-max decoding -- is not rnnt_greedy at max_symbols=1: after an emission
    greedy looks at the same frame again (and is forced to take its blank), this search does not.
    Everything that can be judged from the arguments is refused before the device is touched.  V is known only from what `output`
    returns, so V >= 2 and blank < V are checked on the first frame's logits: behind the first joint launch and the first `output`,
    in front of the first select launch (whose entry refuses the same)."""
    who = 'rnnt_beam'
    if pe.dim() != 3:
        raise ValueError('%s: pe must be [B, T, J], got %s' % (who, tuple(pe.shape)))
    B, T, J = pe.shape
    if J < 4 or J % 4:
        raise ValueError('%s: J=%d must be a positive multiple of 4' % (who, J))
    rnnt_beam_limits(who, beam_width, max_len)
    if int(blank) < 0:
        raise ValueError('%s: blank=%r must be >= 0' % (who, blank))
    W = beam_width
    R = B * W
    if B < 1 or T < 1 or R > 65535:
        raise ValueError('%s: pe [B, T, J] = %s at beam_width=%d needs B, T >= 1 and B * beam_width <= 65535 rows' % (who, (B, T, J), W))
    _rnnt_int_vector(who, 'enc_len', enc_len, B)
    _cuda(pe, enc_len)
    if pe.dtype != torch.float32:
        raise L.OtransHipError('%s: pe must be f32, got %s' % (who, pe.dtype))
    pe, dev, lib = pe.contiguous(), pe.device, L.load()
    half = _ops.is_half()
    el = _len32(enc_len)
    # the beam, twice: frame t reads half t & 1 and writes the other
    score = [torch.full((R,), float('-inf'), dtype=torch.float32, device=dev) for _ in range(2)]
    score[0].view(B, W)[:, 0] = 0.0
    n = [torch.zeros((R,), dtype=torch.int32, device=dev) for _ in range(2)]
    tokens = [torch.zeros((R, max_len), dtype=torch.int64, device=dev) for _ in range(2)]
    frames = [torch.zeros((R, max_len), dtype=torch.int32, device=dev) for _ in range(2)]
    parent, emit = (torch.zeros((R,), dtype=torch.int32, device=dev) for _ in range(2))
    step_tok = torch.full((R,), int(blank), dtype=torch.int64, device=dev)
    h0, c0, pg0 = predictor_step(torch.full((B, 1), int(bos), dtype=torch.int64, device=dev), None, None)
    nl = len(h0)

    def items(hs, cs, g):
        out = list(hs) + list(cs) + [g]
        if half:
            out += [_ops.lp_of(x) for x in hs]
        return out
    first = items(h0, c0, pg0.contiguous())
    if any(x is None or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != B for x in first):
        raise L.OtransHipError('%s: predictor_step must return contiguous [rows, width] states (with their 16-bit twins in the 16-bit modes)' % who)
    # the committed predictor state, twice, on R rows: the state after BOS sits in slot 0 of every utterance
    state = [[torch.zeros((R, x.shape[1]), dtype=x.dtype, device=dev) for x in first] for _ in range(2)]
    for buf, x in zip(state[0], first):
        buf.view(B, W, -1)[:, 0] = x

    def lists(bufs):
        hs = [_ops.attach_lp(bufs[k], bufs[2 * nl + 1 + k]) if half else bufs[k] for k in range(nl)]
        return hs, bufs[nl:2 * nl], bufs[2 * nl]
    # the gather and commit entries take at most 16 items a call: 3 per layer + 1 in the 16-bit modes, so a deep predictor takes more
    cuts = [(i, min(i + 16, len(first))) for i in range(0, len(first), 16)]
    nbytes = [(C.c_int32 * (j - i))(*[x.shape[1] * x.element_size() for x in first[i:j]]) for i, j in cuts]
    ptrs = [[(C.c_void_p * (j - i))(*[x.data_ptr() for x in state[s][i:j]]) for i, j in cuts] for s in range(2)]
    z = torch.empty((R, J), dtype=torch.float32, device=dev)
    z16 = torch.empty((R, J), dtype=_ops.half_dtype(), device=dev) if half else None
    st = _stream()
    for t in range(T):
        cur, nxt = t & 1, 1 - (t & 1)
        h, c, pg = lists(state[cur])
        L.check(lib.otr_rnnt_beam_joint(_p(pe), _p(pg), _p(score[cur]), _p(el), B, W, T, t, J, _p(z), _p(z16), st), 'otr_rnnt_beam_joint')
        logits = output(_ops.attach_lp(z, z16))
        V = logits.shape[-1]
        if t == 0 and (V < 2 or not 0 <= int(blank) < V):
            raise ValueError('%s: V=%d must be >= 2 and blank=%r inside [0, V)' % (who, V, blank))
        lg, ld = _rows_in_place(logits, V)
        L.check(lib.otr_rnnt_beam_select(_p(lg), ld, _p(el), B, W, T, t, V, int(blank), max_len, _p(score[cur]), _p(n[cur]), _p(tokens[cur]),
                                         _p(frames[cur]), _p(score[nxt]), _p(n[nxt]), _p(tokens[nxt]), _p(frames[nxt]), _p(parent),
                                         _p(step_tok), _p(emit), st), 'otr_rnnt_beam_select')
        for k, (i, j) in enumerate(cuts):
            L.check(lib.otr_rnnt_beam_gather(_p(parent), ptrs[cur][k], ptrs[nxt][k], nbytes[k], j - i, B, W, st), 'otr_rnnt_beam_gather')
        h, c, _ = lists(state[nxt])
        h1, c1, pg1 = predictor_step(step_tok.view(R, 1), h, c)
        src = items(h1, c1, pg1.contiguous())
        for k, (i, j) in enumerate(cuts):
            src_p = (C.c_void_p * (j - i))(*[x.data_ptr() for x in src[i:j]])
            L.check(lib.otr_rnnt_greedy_commit(_p(emit), src_p, ptrs[nxt][k], nbytes[k], j - i, R, st), 'otr_rnnt_greedy_commit')
    fin = T & 1
    # a slot may hold a shorter hypothesis than the one it held two frames ago: what that left behind the length is cleared once, here
    behind = torch.arange(max_len, device=dev).view(1, -1) >= n[fin].view(-1, 1)
    return (tokens[fin].masked_fill_(behind, 0).view(B, W, max_len), n[fin].view(B, W), score[fin].view(B, W),
            frames[fin].masked_fill_(behind, 0).view(B, W, max_len))


# ------------------------------------------------------------------ knowledge distillation (csrc/distill.hip)
DISTILL_MAX_V, DISTILL_MAX_K = 8192, 128


class DistillLossFn(torch.autograd.Function):
    """The temperature-scaled KL divergence of student logits [B, T, V] from a teacher (include/otrans_hip.h otr_distill_loss): dense
    (`teacher` [B, T, V]) or sparse (`top_val`, `top_idx` [B, T, K]), + its gradient into the student's logits in the same call when
    they need one, like MwerLossFn: the head of a row-padded product is read in place, the gradient leaves as the head of a zero-tailed
    [R, V8] buffer, `gscale` (a device scalar; None = 1) rides in the written gradient, and backward multiplies by the incoming gradient
    unless that is the cached unit seed of ops.backward.  Returns (loss, row_kl [B, T]); only loss is differentiable, and only with
    respect to the student.  The gradient is fp32."""

    @staticmethod
    def forward(ctx, student, teacher, top_val, top_idx, lengths, temperature, gscale):
        B, T, V = student.shape
        lg, ld = _rows_in_place(student, V)
        R, ldd = lg.shape[0], _grad_width(ld, V)
        need = ctx.needs_input_grad[0]
        f32 = _f32(lg.device)
        loss, row_kl = f32(), f32(B, T)
        dlogits = f32(R, ldd) if need else None
        K, ld_t, tg = 0, 0, None
        if teacher is not None:
            tg, ld_t = _rows_in_place(teacher, V)
        else:
            K = top_val.shape[-1]
            top_val, top_idx = top_val.reshape(-1, K).contiguous(), top_idx.reshape(-1, K).contiguous()
        lib = L.load()
        ws = f32(max(lib.otr_distill_workspace_floats(B, T), 4))
        L.check(_timed('distill_loss %dx%dx%d%s' % (B, T, V, ' K=%d' % K if K else ''),
                       {'bytes': R * ((V if K else 2 * V) + (ldd if need else 0)) * 4},
                       lambda: lib.otr_distill_loss(_p(lg), ld, _p(tg), ld_t, _p(top_val), _p(top_idx), K, _p(lengths), B, T, V,
                                                    float(temperature), _p(gscale), _p(loss), _p(row_kl), _p(dlogits), ldd, _p(ws),
                                                    ws.numel(), _stream())), 'otr_distill_loss')
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.V = student.shape, V
        ctx.mark_non_differentiable(row_kl)
        return loss, row_kl

    @staticmethod
    def backward(ctx, g, *_):
        return _saved_logits_grad(ctx, g), None, None, None, None, None, None


def _distill_args(who, student, lengths, temperature):
    """the checks both forms share; returns (B, T, V)"""
    if student.dim() != 3:
        raise ValueError('%s: student logits must be [B, T, V], got %s' % (who, tuple(student.shape)))
    B, T, V = student.shape
    if not 1 <= V <= DISTILL_MAX_V:
        raise ValueError('%s: vocabulary V=%d must be in [1, %d]' % (who, V, DISTILL_MAX_V))
    if T < 1 or B * T >= 1 << 30:
        raise ValueError('%s: B*T = %d*%d must be in [0, 2^30) with T >= 1' % (who, B, T))
    if lengths.numel() != B:
        raise ValueError('%s: lengths must hold B = %d entries, got %s' % (who, B, tuple(lengths.shape)))
    tau = float(temperature)
    if not (tau > 0 and tau != float('inf')):
        raise ValueError('%s: temperature=%r must be finite and > 0' % (who, temperature))
    return B, T, V


def _distill_run(who, student, teacher, top_val, top_idx, lengths, temperature, grad_scale):
    _cuda(student, teacher, top_val, top_idx, lengths, grad_scale)
    if student.dtype != torch.float32 or lengths.dtype not in (torch.int32, torch.int64) or (
            grad_scale is not None and grad_scale.dtype != torch.float32):
        raise L.OtransHipError('%s: student f32, lengths int32 (or int64), grad_scale f32 expected' % who)
    B, T = student.shape[:2]
    if B == 0:
        return student.new_zeros(()), student.new_zeros((0, T))
    return DistillLossFn.apply(student, teacher, top_val, top_idx, _len32(lengths), float(temperature), grad_scale)


def distill_loss(student_logits, teacher_logits, lengths, temperature=1.0, grad_scale=None):
    """Knowledge-distillation loss against a dense teacher (include/otrans_hip.h otr_distill_loss): tau^2 / n_live times the sum over
    the live rows (b, i < lengths[b]) of KL(softmax(teacher / tau) || softmax(student / tau)).  student_logits f32 [B, T, V] with unit
    stride along the vocabulary (a view with a longer row stride, such as the head of a row-padded product, is read in place);
    teacher_logits f32 of the same shape, it takes no gradient; lengths int32 [B] on the device.  grad_scale: a device scalar the
    gradient into the student's logits is multiplied by (the loss scale), None = 1.  Returns (loss, row_kl [B, T] detached).
    At most three launches on the current stream, no host synchronisation, the same bits on every run: capturable."""
    B, T, V = _distill_args('distill_loss', student_logits, lengths, temperature)
    if tuple(teacher_logits.shape) != (B, T, V):
        raise ValueError('distill_loss: teacher logits %s do not match the student\'s %s' % (tuple(teacher_logits.shape), (B, T, V)))
    _cuda(student_logits, teacher_logits)
    if teacher_logits.dtype != torch.float32:
        raise L.OtransHipError('distill_loss: teacher logits must be f32, got %s' % teacher_logits.dtype)
    return _distill_run('distill_loss', student_logits, teacher_logits.detach(), None, None, lengths, temperature, grad_scale)


def distill_loss_topk(student_logits, top_val, top_idx, lengths, temperature=1.0, grad_scale=None):
    """distill_loss against a sparse teacher: top_val f32 / top_idx int32 [B, T, K] (what topk_rows returns; logits or log-probs), K <=
    DISTILL_MAX_K.  The teacher's distribution of a row is the softmax of its listed values (index in [0, V); the top-K mass is
    renormalised) and zero elsewhere; a row that lists nothing takes no part.  Indices within a row must be distinct."""
    B, T, V = _distill_args('distill_loss_topk', student_logits, lengths, temperature)
    if top_val.dim() != 3 or tuple(top_val.shape[:2]) != (B, T) or top_idx.shape != top_val.shape:
        raise ValueError('distill_loss_topk: top_val and top_idx must both be [B, T, K] = [%d, %d, K], got %s and %s'
                         % (B, T, tuple(top_val.shape), tuple(top_idx.shape)))
    K = top_val.shape[2]
    if not 1 <= K <= DISTILL_MAX_K:
        raise ValueError('distill_loss_topk: K=%d entries per row must be in [1, %d]' % (K, DISTILL_MAX_K))
    _cuda(student_logits, top_val, top_idx)
    if top_val.dtype != torch.float32 or top_idx.dtype != torch.int32:
        raise L.OtransHipError('distill_loss_topk: top_val f32 and top_idx int32 expected, got %s and %s' % (top_val.dtype, top_idx.dtype))
    return _distill_run('distill_loss_topk', student_logits, None, top_val.detach(), top_idx, lengths, temperature, grad_scale)


def topk_rows(x, lengths, K):
    """The K largest entries of every row of x f32 [B, T, V] (include/otrans_hip.h otr_ctc_topk): (val f32 [B, T, K] descending, idx
    int32 [B, T, K], ties to the lower index).  Rows at or past lengths[b] are left as zeros -- K copies of (0.0, index 0), which is
    not a legal sparse row (the indices repeat): hand distill_loss_topk the same lengths, so that it never reads them.  The producer
    of sparse teachers for distill_loss_topk: 2K numbers per frame instead of V.  One launch, no host synchronisation."""
    if x.dim() != 3:
        raise ValueError('topk_rows: x must be [B, T, V], got %s' % (tuple(x.shape),))
    B, T, V = x.shape
    K = int(K)
    if not 1 <= V <= DISTILL_MAX_V:
        raise ValueError('topk_rows: V=%d must be in [1, %d]' % (V, DISTILL_MAX_V))
    if not 1 <= K <= min(DISTILL_MAX_K, V):
        raise ValueError('topk_rows: K=%d must be in [1, min(%d, V=%d)]' % (K, DISTILL_MAX_K, V))
    if T < 1 or lengths.numel() != B:
        raise ValueError('topk_rows: T=%d must be >= 1 and lengths hold B = %d entries' % (T, B))
    _cuda(x, lengths)
    if x.dtype != torch.float32:
        raise L.OtransHipError('topk_rows: x must be f32, got %s' % x.dtype)
    x = x.detach()
    if not (x.stride(2) == 1 and x.stride(1) >= V and x.stride(0) == T * x.stride(1)):
        x = x.contiguous()
    val = torch.zeros((B, T, K), dtype=torch.float32, device=x.device)
    idx = torch.zeros((B, T, K), dtype=torch.int32, device=x.device)
    if B:
        L.check(L.load().otr_ctc_topk(_p(x), x.stride(1), _p(_len32(lengths)), B, T, V, K, _p(val), _p(idx), _stream()), 'otr_ctc_topk')
    return val, idx
