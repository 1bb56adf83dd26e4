"""Named cases of the transducer loss: the smallest shapes at which the kernels of csrc/rnnt.hip can still go wrong.  Every case is
built from a seed and returns float32 logits [B, T, U1, V], int64 labels [B, >= U1 - 1] and the two length vectors (int32).

  tiny         B 3, T 5, U1 4, V 5            plumbing; V below one wavefront
  ragged       B 4, T 9, U1 7, V 37           lengths (9,6), (1,0), (1,6), (7,0): T_b = 1, U_b = 0, a single row, a single column
  wave_edges   B 6, T 6, U1 256, V 11         U_b in {62, 63, 64, 127, 128, 255}: live columns on both sides of every wavefront
                                              boundary of the lattice pass, up to the advertised limit
  long_t       B 2, T 300, U1 3, V 8          diagonals far outnumber columns; one utterance with T_b = 299
  vocab_<V>    B 2, T 3, U1 3, V in {63, 64, 65, 4233}   row-pass tails, odd row starts, several strides per lane
  peaked       tiny with the logits scaled by 40        saturated softmax
  guarded      B 6, T 4, U1 4, V 7            0: a label equal to V (position 0), 1: valid, 2: T_b = 0, 3: valid,
                                              4: U_b = RNNT_MAX_TGT + 1 by length only, 5: a blank inside the labels
"""
import functools

import torch

RNNT_MAX_TGT = 255


def _make(seed, B, T, U1, V, enc_len, tgt_len, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, U1, V), generator=g, dtype=torch.float32) * scale
    labels = torch.randint(1, V, (B, max(U1 - 1, 1)), generator=g, dtype=torch.int64)
    return {'logits': logits, 'labels': labels, 'enc_len': torch.tensor(enc_len, dtype=torch.int32),
            'tgt_len': torch.tensor(tgt_len, dtype=torch.int32)}


def tiny():
    return _make(11, 3, 5, 4, 5, [5, 4, 3], [3, 2, 1])


def ragged():
    return _make(12, 4, 9, 7, 37, [9, 1, 1, 7], [6, 0, 6, 0])


def wave_edges():
    return _make(13, 6, 6, 256, 11, [6, 5, 6, 3, 6, 6], [62, 63, 64, 127, 128, 255])


def long_t():
    return _make(14, 2, 300, 3, 8, [299, 300], [2, 1])


def vocab(V):
    return _make(15 + V, 2, 3, 3, V, [3, 2], [2, 1])


def peaked():
    c = tiny()
    c['logits'] = c['logits'] * 40
    return c


def guarded():
    V = 7
    c = _make(16, 6, 4, 4, V, [4, 3, 0, 4, 4, 4], [3, 2, 2, 1, RNNT_MAX_TGT + 1, 3])
    c['labels'][0, 0] = V            # read unguarded it would be a wrong but in-bounds element of the next row
    c['labels'][5, 1] = 0
    return c


GUARDED_DEAD = (0, 2, 4, 5)          # the utterances of `guarded` that take no part

def model_config(vocab=100, joint_size=64):
    """TransducerModel on the C1 frontend and encoder (d 64, 2 blocks): predictor E 64 / H 64 / 2 layers"""
    from opentransformer_amd import synthetic as syn
    m = syn.c1_model(0.0)
    m.pop('decoder', None)
    m.pop('decoder_type', None)
    m.update(vocab_size=vocab, joint_size=joint_size, predictor=dict(embedding_size=64, hidden_size=64, num_layers=2, dropout=0.0))
    return m


def reference(c, dtype):
    """rnnt_loss_ref and its autograd gradient on the case's logits in `dtype`: (loss, nll [B], valid [B], d loss / d logits)"""
    from tests import rnnt_ref as rr
    x = c['logits'].detach().clone().to(dtype).requires_grad_(True)
    loss, nll, valid = rr.rnnt_loss_ref(x, c['enc_len'], c['labels'], c['tgt_len'])
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), nll.detach(), valid, g


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """the float64 reference of a case, computed once and shared; do not write into it"""
    return reference(build(name), torch.float64)


@functools.lru_cache(maxsize=None)
def closed_form_of(name):
    """(the closed-form gradient, the occupancies exp(alpha + beta - lnP) / B [B, T, U1]) of a case in float64, computed once"""
    from tests import rnnt_ref as rr
    c = build(name)
    return rr.rnnt_grad_ref(c['logits'].double(), c['enc_len'], c['labels'], c['tgt_len'], with_occupancy=True)


def rowsum_rel(g, occ):
    """|sum_v g| of every row over max(sum_v |g|, occupancy) [B, T, U1] (0 where the row is zero).  The occupancy is in the
    denominator because a row is p * occ minus two terms that add up to occ: where the softmax is saturated the row is smaller than
    its terms by many orders, and its sum is then only as small as the rounding of those terms, in any precision."""
    g = g.double()
    den = torch.maximum(g.abs().sum(-1), occ.double())
    return torch.where(den > 0, g.sum(-1).abs() / den.clamp_min(1e-300), den)


def slab_rel(g, ref):
    """relative Frobenius distance per utterance slab (0 where both are zero)"""
    B = ref.shape[0]
    d = (g.double() - ref.double()).reshape(B, -1).norm(dim=1)
    n = ref.double().reshape(B, -1).norm(dim=1)
    return torch.where(n > 0, d / n.clamp_min(1e-300), d)


@functools.lru_cache(maxsize=None)
def floor_of(name):
    """the distance of the float32 run of the restatement from its float64 run, per utterance: {'nll' (relative), 'grad' (slab_rel)},
    and tiny [B] = (T_b + U_b) * eps_fp32 * max |lp_b| over the live rows: what the roundings of the T_b + U_b log-domain additions
    along a path may add up to, in the log domain, hence relative in the gradient"""
    c = build(name)
    _, nll64, valid, g64 = reference_of(name)
    _, nll32, _, g32 = reference(c, torch.float32)
    B = nll64.shape[0]
    tiny = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        if bool(valid[b]):
            Tb, Ub = int(c['enc_len'][b]), int(c['tgt_len'][b])
            lp = torch.log_softmax(c['logits'][b, :Tb, :Ub + 1].detach().double(), dim=-1)
            tiny[b] = (Tb + Ub) * float(torch.finfo(torch.float32).eps) * float(lp.abs().max())
    nll_floor = (nll32.double() - nll64).abs() / nll64.abs().clamp_min(1e-300)
    return {'nll': torch.where(valid, nll_floor, torch.zeros_like(nll_floor)), 'grad': slab_rel(g32, g64), 'tiny': tiny}


CASES = {'tiny': tiny, 'ragged': ragged, 'wave_edges': wave_edges, 'long_t': long_t, 'vocab_63': lambda: vocab(63),
         'vocab_64': lambda: vocab(64), 'vocab_65': lambda: vocab(65), 'vocab_4233': lambda: vocab(4233), 'peaked': peaked,
         'guarded': guarded}
