"""The cases of the CTC-MWER tests, shared by tests/test_ctc_mwer.py (CPU) and tests/test_gpu_ctc_mwer.py, and the independent
composition from torch ops they are compared with.

Recipe of a main case: unit-variance gaussian logits (a standard deviation of 3 collapses the posterior onto one slot and would make the
test vacuous), slot 0 is the reference, slot n the reference with 1 + n % 3 random substitutions, errors their true edit distance.
Condition, asserted for every main case: at least a third of the live slots carry |P_n (W_n - E_b)| > 1e-3."""
import numpy as np
import torch
import torch.nn.functional as F

from opentransformer_amd.tools import edit_distance
from tests import ctc_mwer_ref as ref

BLANK = 0
CARRY, CARRY_SHARE = 1e-3, 1.0 / 3.0


def carrying_share(case):
    """the share of the live slots with |P_n (W_n - E_b)| > CARRY at scale 1 (0 without a live slot)"""
    f = ref.forward(case['logits'], case['in_len'], case['hyps'], case['hyp_len'], case['errors'])
    live = f['live']
    w = np.abs(f['post'] * (case['errors'] - f['utt_err'][:, None]))
    return float((w[live] > CARRY).mean()) if live.any() else 0.0


def main_case(seed, B, T, V, N, max_lab=8, in_len=None, lab_len=None, width=None):
    """dict of numpy arrays: logits f64 [B, T, V], in_len [B] (below T and equal to T), hyps [B, N, width] padded with -1, hyp_len,
    errors [B, N], ref [B, max_lab] padded with -1, ref_len [B]"""
    rng = np.random.default_rng(seed)
    width = width or max_lab
    logits = rng.normal(size=(B, T, V))
    in_len = np.array(in_len if in_len is not None else [T if b % 2 == 0 else T - 3 - b for b in range(B)], np.int32)
    lab_len = lab_len if lab_len is not None else [max_lab if b == 0 else int(rng.integers(2, max_lab + 1)) for b in range(B)]
    hyps = -np.ones((B, N, width), np.int64)
    hyp_len = np.zeros((B, N), np.int32)
    errors = np.zeros((B, N), np.int32)
    refs = -np.ones((B, max_lab), np.int64)
    for b in range(B):
        L = lab_len[b]
        truth = rng.integers(1, V, size=L)
        refs[b, :L] = truth
        for n in range(N):
            h = truth.copy()
            if n:
                for i in rng.choice(L, size=min(1 + n % 3, L), replace=False):
                    h[i] = 1 + (h[i] - 1 + rng.integers(1, V - 1)) % (V - 1)        # another label, never the blank
            hyps[b, n, :L], hyp_len[b, n] = h, L
            errors[b, n] = edit_distance(truth.tolist(), h.tolist())
    case = {'logits': logits, 'in_len': in_len, 'hyps': hyps, 'hyp_len': hyp_len, 'errors': errors, 'ref': refs,
            'ref_len': np.array(lab_len, np.int32)}
    if N > 1:
        share = carrying_share(case)
        assert share >= CARRY_SHARE, 'vacuous case: only %.3f of the live slots carry a gradient' % share
    return case


def with_edges(case, V):
    """a copy of a B = 4 main case with the edge cases planted where N leaves room: utterance 0 gets a hypothesis with a repeated label
    (a a: needs the blank between) and an empty one, utterance 1 one dead slot of each kind that concerns a slot alone (a negative
    error, a length past the bound, a label >= V), utterance 2 few frames and a hypothesis with more labels than frames, utterance 3
    in_len 0: wholly dead.  Returns (case, dead bool [B, N]: what has to come out not live)."""
    c = {k: v.copy() for k, v in case.items()}
    B, N, W = c['hyps'].shape
    assert B == 4
    dead = np.zeros((B, N), bool)

    def put(b, n, labels):
        c['hyps'][b, n] = -1
        c['hyps'][b, n, :len(labels)] = labels
        c['hyp_len'][b, n] = len(labels)
        c['errors'][b, n] = edit_distance(c['ref'][b, :c['ref_len'][b]].tolist(), list(labels))
    if N >= 2:
        a = int(c['ref'][0, 0])
        put(0, N - 1, [a, a] + c['ref'][0, 2:c['ref_len'][0]].tolist())
        c['errors'][1, N - 1] = -3
        dead[1, N - 1] = True
    if N >= 5:
        put(0, N - 2, [])
        c['hyp_len'][1, N - 2] = 128
        c['hyps'][1, N - 3, 1] = V
        dead[1, N - 2] = dead[1, N - 3] = True
    # utterance 2: 4 frames, a reference of 2 labels; its last slot holds 6 labels (slot 0 at N = 1: the utterance is dead then)
    c['in_len'][2] = 4
    c['ref'][2, 2:] = -1
    c['ref_len'][2] = 2
    for n in range(N):
        put(2, n, [int(c['ref'][2, 0]), 1 + (int(c['ref'][2, 1]) - 1 + n) % (V - 1)])
    put(2, N - 1, [1 + i % (V - 1) for i in range(6)])
    dead[2, N - 1] = True
    c['in_len'][3] = 0
    dead[3] = True
    return c, dead


def big_case(seed=5):
    """B 2, T 300, V 100, N 5, 127 labels: S = 255, the whole workgroup of states.  The rows are 130 wide and slot 4 of utterance 1
    claims 128 labels -- they would fit into the frames, the bound of 127 makes the slot dead."""
    c = main_case(seed, 2, 300, 100, 5, max_lab=127, in_len=[300, 290], lab_len=[127, 127], width=130)
    c['hyps'][1, 4, 127] = 7
    c['hyp_len'][1, 4] = 128
    dead = np.zeros((2, 5), bool)
    dead[1, 4] = True
    return c, dead


def compose_torch(case, live, ctc_weight, scale, with_ref, dtype=torch.float64, g=1.0):
    """The loss composed from torch ops on the CPU: F.ctc_loss(reduction='none') per hypothesis, a softmax over the live slots, the
    expected errors, F.ctc_loss on the reference, autograd.  `live` bool [B, N] says which slots take part (a dead slot is scored
    with an empty label row and masked out; liveness itself is the restatement's business).  Returns (loss, mwer, ctc, dlogits), the
    gradient times g."""
    x = torch.tensor(case['logits'], dtype=dtype, requires_grad=True)
    B, T, V = x.shape
    N = live.shape[1]
    lp = F.log_softmax(x, dim=-1).transpose(0, 1)                      # [T, B, V]
    il = torch.tensor(np.clip(case['in_len'], 1, T).astype(np.int64))  # an utterance without frames has no live slot: any length does
    live_t = torch.tensor(live)
    lls = []
    for n in range(N):
        tl = torch.tensor(np.where(live[:, n], case['hyp_len'][:, n], 0).astype(np.int64))
        tg = torch.tensor(np.where(case['hyps'][:, n] < 0, 1, case['hyps'][:, n])).clamp(max=V - 1)
        lls.append(-F.ctc_loss(lp, tg, il, tl, blank=BLANK, reduction='none', zero_infinity=False))
    s = torch.stack(lls, dim=1)                                        # [B, N]
    s = torch.where(live_t, scale * s, torch.full_like(s, float('-inf')))
    any_live = live_t.any(dim=1)
    s = torch.where(any_live[:, None], s, torch.zeros_like(s))         # no nan out of an all -inf row; masked below
    post = torch.softmax(s, dim=1) * live_t
    e = (post * torch.tensor(case['errors'] * live, dtype=dtype)).sum(dim=1)
    b_live = int(any_live.sum())
    mwer = (e * any_live).sum() / b_live if b_live else x.sum() * 0
    ctc = x.sum() * 0
    if with_ref:
        rl = torch.tensor(case['ref_len'].astype(np.int64))
        rg = torch.tensor(np.where(case['ref'] < 0, 1, case['ref']))
        il0 = torch.tensor(np.clip(case['in_len'], 0, T).astype(np.int64))
        keep = il0 > 0                                                 # F.ctc_loss wants a frame; without one there is no alignment
        nll = F.ctc_loss(lp, rg, il, rl, blank=BLANK, reduction='none', zero_infinity=True)
        ctc = (torch.where(keep, nll, torch.zeros_like(nll)) / rl.clamp(min=1)).sum() / B
    loss = mwer + ctc_weight * ctc
    (d,) = torch.autograd.grad(loss * g, x)
    return loss.detach(), mwer.detach(), ctc.detach(), d.numpy()
