"""The transducer's definitions restated in plain torch, dtype-generic (run them in float64 for a reference, in float32 for the
rounding floor of that very computation).  include/otrans_hip.h (otr_rnnt_*) states the same in words.  blank = 0.

  rnnt_loss_ref      (loss, nll [B], valid [B]); differentiable, one logaddexp per anti-diagonal
  rnnt_lattice_ref   alpha, beta [T_b, U_b + 1] and lp of ONE utterance (cell loops; no autograd)
  rnnt_grad_ref      d loss / d logits by the closed form of the header
  joint_ref          tanh(pe[:, :, None] + pg[:, None]) with zeros outside the lengths
  rnnt_greedy_ref    the greedy decoder of one utterance, a plain loop
"""
import torch

BLANK = 0
RNNT_MAX_TGT = 255
_NEG = -1e30          # stands in for -inf inside the differentiable sweep: logaddexp(_NEG, x) == x with a zero gradient, never a NaN


def is_guarded(Tb, Ub, labels_b, T, U1, V, max_tgt=RNNT_MAX_TGT):
    if Tb <= 0 or Ub < 0 or Ub > max_tgt or Tb > T or Ub + 1 > U1:
        return True
    y = labels_b[:Ub]
    return bool(((y < 1) | (y >= V)).any())


def _alpha_final(lp, y, Tb, Ub):
    """ln P of one utterance from lp [Tb, Ub + 1, V]: alpha swept along the anti-diagonals, every diagonal one vector over u"""
    lpb = lp[:, :, BLANK]                                                       # [Tb, Ub + 1]
    lpl = lp[:, :Ub, :].gather(2, y.view(1, Ub, 1).expand(Tb, Ub, 1))[..., 0] if Ub else lp.new_zeros((Tb, 0))
    u = torch.arange(Ub + 1)
    prev = torch.where(u == 0, lp.new_zeros(Ub + 1), lp.new_full((Ub + 1,), _NEG))
    for d in range(1, Tb + Ub):
        t = d - u
        live = (t >= 0) & (t < Tb)
        has_up, has_left = live & (t >= 1), live & (u >= 1)
        up = prev + lpb[(t - 1).clamp(0, Tb - 1), u]
        if Ub:
            left = torch.cat((prev.new_full((1,), _NEG), prev[:-1])) + torch.cat((prev.new_zeros(1), lpl[t.clamp(0, Tb - 1)[1:], u[1:] - 1]))
        else:
            left = prev.new_full((1,), _NEG)
        neg = prev.new_full((), _NEG)
        cur = torch.logaddexp(torch.where(has_up, up, neg), torch.where(has_left, left, neg))
        prev = torch.where(live, cur, neg)
    return prev[Ub] + lpb[Tb - 1, Ub]


def rnnt_loss_ref(logits, enc_len, labels, tgt_len, max_tgt=RNNT_MAX_TGT):
    """logits [B, T, U1, V] raw, labels int64 [B, >= U1 - 1]; (loss = mean over ALL B of nll, nll [B], valid bool [B]).  A guarded
    utterance has nll 0 (connected to the graph with a zero gradient)."""
    B, T, U1, V = logits.shape
    nll, valid = [], []
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(tgt_len[b])
        if is_guarded(Tb, Ub, labels[b], T, U1, V, max_tgt):
            nll.append(logits[b, 0, 0, 0] * 0)
            valid.append(False)
            continue
        lp = torch.log_softmax(logits[b, :Tb, :Ub + 1], dim=-1)
        nll.append(-_alpha_final(lp, labels[b, :Ub], Tb, Ub))
        valid.append(True)
    nll = torch.stack(nll)
    return nll.sum() / B, nll, torch.tensor(valid)


@torch.no_grad()
def rnnt_lattice_ref(logits_b, y, Tb, Ub):
    """(alpha, beta [Tb, Ub + 1], lp [Tb, Ub + 1, V]) of one valid utterance, cell by cell"""
    lp = torch.log_softmax(logits_b[:Tb, :Ub + 1], dim=-1)
    ninf = lp.new_full((), float('-inf'))
    alpha = lp.new_full((Tb, Ub + 1), float('-inf'))
    beta = lp.new_full((Tb, Ub + 1), float('-inf'))
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[t, u] = 0
                continue
            a = alpha[t - 1, u] + lp[t - 1, u, BLANK] if t > 0 else ninf
            e = alpha[t, u - 1] + lp[t, u - 1, y[u - 1]] if u > 0 else ninf
            alpha[t, u] = torch.logaddexp(a, e)
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                beta[t, u] = lp[t, u, BLANK]
                continue
            a = beta[t + 1, u] + lp[t, u, BLANK] if t + 1 < Tb else ninf
            e = beta[t, u + 1] + lp[t, u, y[u]] if u < Ub else ninf
            beta[t, u] = torch.logaddexp(a, e)
    return alpha, beta, lp


@torch.no_grad()
def rnnt_grad_ref(logits, enc_len, labels, tgt_len, max_tgt=RNNT_MAX_TGT, with_occupancy=False):
    """d rnnt_loss_ref / d logits by the closed form: per live row p * exp(alpha + beta - lnP) minus the blank's and the label's
    occupancies, 1 / B in front; zeros on every other row.  with_occupancy: also occ [B, T, U1] = exp(alpha + beta - lnP) / B, the
    size of the terms a row is the difference of (a saturated row is far smaller than its terms)"""
    B, T, U1, V = logits.shape
    g = torch.zeros_like(logits)
    occ = logits.new_zeros((B, T, U1))
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(tgt_len[b])
        if is_guarded(Tb, Ub, labels[b], T, U1, V, max_tgt):
            continue
        y = labels[b, :Ub]
        alpha, beta, lp = rnnt_lattice_ref(logits[b], y, Tb, Ub)
        lnP = beta[0, 0]
        for t in range(Tb):
            for u in range(Ub + 1):
                row = lp[t, u].exp() * (alpha[t, u] + beta[t, u] - lnP).exp()
                bn = beta[t + 1, u] if t + 1 < Tb else (beta.new_zeros(()) if u == Ub else beta.new_full((), float('-inf')))
                row[BLANK] -= (alpha[t, u] + lp[t, u, BLANK] + bn - lnP).exp()
                if u < Ub:
                    row[y[u]] -= (alpha[t, u] + lp[t, u, y[u]] + beta[t, u + 1] - lnP).exp()
                g[b, t, u] = row / B
                occ[b, t, u] = (alpha[t, u] + beta[t, u] - lnP).exp() / B
    return (g, occ) if with_occupancy else g


def joint_ref(pe, pg, enc_len, tgt_len):
    """z [B, T, U1, J] = tanh(pe[b,t] + pg[b,u]) for t < T_b, u <= U_b (lengths clamped), zeros elsewhere; NaN outside the lengths of
    pe / pg does not reach the result"""
    B, T, J = pe.shape
    U1 = pg.shape[1]
    z = pe.new_zeros((B, T, U1, J))
    for b in range(B):
        Tb, Un = min(max(int(enc_len[b]), 0), T), min(max(int(tgt_len[b]) + 1, 0), U1)
        z[b, :Tb, :Un] = torch.tanh(pe[b, :Tb, None, :] + pg[b, None, :Un, :])
    return z


@torch.no_grad()
def rnnt_greedy_ref(pe_b, Tb, predict, joint_logits, max_symbols, max_len, bos=1):
    """Greedy decoding of ONE utterance.  pe_b [T, J]; predict(token, state) -> (pg [J], state) (state None: zero);
    joint_logits(pe_t, pg) -> logits [V].  Returns (tokens, frames, score, min_gap): min_gap the smallest top-1 / top-2 logit gap
    over every decision taken."""
    tokens, frames, score, gap = [], [], 0.0, float('inf')
    pg, state = predict(bos, None)
    t, count = 0, 0
    while t < Tb and len(tokens) < max_len:
        lg = joint_logits(pe_b[t], pg)
        lp = torch.log_softmax(lg, dim=-1)
        top = torch.topk(lg, 2).values
        gap = min(gap, float(top[0] - top[1]))
        k = int(torch.argmax(lg))
        if k != BLANK and count < max_symbols:
            tokens.append(k)
            frames.append(t)
            score += float(lp[k])
            count += 1
            pg, state = predict(k, state)
        else:
            score += float(lp[BLANK])
            t += 1
            count = 0
    return tokens, frames, score, gap


def transducer_weights(vocab=100, emb=64, hidden=64, layers=2, enc=64, joint=64, seed=22):
    """the predictor's and the joint's weights under TransducerModel's state_dict keys, float32, filled like every other test model"""
    from opentransformer_amd import synthetic as syn
    sd = {'predictor.embedding.weight': torch.empty(vocab, emb)}
    for k in range(layers):
        sd['predictor.rnn.weight_ih_l%d' % k] = torch.empty(4 * hidden, emb if k == 0 else hidden)
        sd['predictor.rnn.weight_hh_l%d' % k] = torch.empty(4 * hidden, hidden)
        sd['predictor.rnn.bias_ih_l%d' % k] = torch.empty(4 * hidden)
        sd['predictor.rnn.bias_hh_l%d' % k] = torch.empty(4 * hidden)
    sd.update({'joint.enc_proj.weight': torch.empty(joint, enc), 'joint.enc_proj.bias': torch.empty(joint),
               'joint.pred_proj.weight': torch.empty(joint, hidden), 'joint.output.weight': torch.empty(vocab, joint),
               'joint.output.bias': torch.empty(vocab)})
    syn.fill_state_dict_(sd, seed)
    return sd


class TransducerRef:
    """The predictor and the joint in plain torch on the weights `sd` (any dtype; leaves that require a gradient receive one):
    torch.nn.Embedding / torch.nn.LSTM semantics and three F.linear."""

    def __init__(self, sd, layers=2):
        self.sd, self.layers = sd, layers
        w = sd['predictor.rnn.weight_ih_l0']
        self.rnn = torch.nn.LSTM(w.shape[1], w.shape[0] // 4, layers, batch_first=True).to(w.dtype)
        self.rnn_params = {k[len('predictor.rnn.'):]: v for k, v in sd.items() if k.startswith('predictor.rnn.')}

    def lstm(self, x, state=None):
        return torch.func.functional_call(self.rnn, self.rnn_params, (x, state))

    def project_encoder(self, memory):
        return torch.nn.functional.linear(memory, self.sd['joint.enc_proj.weight'], self.sd['joint.enc_proj.bias'])

    def joint_logits(self, pe, pg):
        """pe [..., J] and pg [..., J] already broadcast against each other"""
        return torch.nn.functional.linear(torch.tanh(pe + pg), self.sd['joint.output.weight'], self.sd['joint.output.bias'])

    def logits(self, memory, tokens_in):
        """memory [B, T, d], tokens_in [B, U1] = [BOS, y_1 .. y_U] -> [B, T, U1, V]"""
        g, _ = self.lstm(torch.nn.functional.embedding(tokens_in, self.sd['predictor.embedding.weight']))
        pg = torch.nn.functional.linear(g, self.sd['joint.pred_proj.weight'])
        return self.joint_logits(self.project_encoder(memory)[:, :, None, :], pg[:, None, :, :])

    def predict(self, token, state):
        """rnnt_greedy_ref's predict: one step on one token -> (pg [J], state)"""
        x = self.sd['predictor.embedding.weight'][token].view(1, 1, -1)
        g, state = self.lstm(x, state)
        return torch.nn.functional.linear(g[0, 0], self.sd['joint.pred_proj.weight']), state
