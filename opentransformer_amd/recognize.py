"""Decode loop: batch beam search with length penalty + LM shallow fusion, CTC greedy
(otrans/recognize/speech2text.py:6-192, recognize/base.py:26-37,104-119, recognize/ctc.py:38-58).

Same constructor arguments and return values as the reference recognizers.  Two decode loops:

* apply_cache=False (the reference's behaviour; it forces this at recognize/speech2text.py:22): per step the
  decoder is re-run over the whole prefix (decoder/transformer.py:185-208), but the scoring is fused on the
  device: the [B*beam, V] log-prob tensor, the LM fusion add, both top-k's, the finished-beam masking and the
  prefix gather are two kernels (otr_beam_topk, otr_beam_prune) instead of ~25 aten launches.
* apply_cache=True (the KV cache is a TODO in the reference, README.md:13): one token per
  hypothesis per step.  Cross-attention K/V are projected once per UTTERANCE (not per beam, not per step);
  self-attention K/V live in write-once caches addressed through a beam-tree ancestor table; the position,
  prefix length and ping-pong state are device-resident, so each step is ONE hipGraph replay
  (decoder + LM + scoring + pruning).  Hypotheses are identical to the re-forward loop.

Both loops keep their beams in a _BeamState and end every step in its `advance` (scoring + prune); a loop only produces the step's
logits.  CachedBeamState is a _BeamState plus what the cache needs.
"""
import ctypes as C
import math
import weakref

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .bias import PhraseBias
from .decode_ops import _rescore_check
from .ngram import NGramLM
from .nn import (BOS, EOS, PAD, LabelSmoothingLoss, PositionalEncoding, TransformerEncoderLayer)

_DECODE_STEP_FUSED = True   # cached beam step on otr_dec_self_step + the fused tail
_DECODE_LAGGED_STOP = True   # cached beam search: the all-finished test lags one step behind the launches (CachedBeamState.run); False = sync after every step
_DECODE_PAIR = True   # cached beam step: the LM's layers ride in the decoder's launches (otr_dec_*_pair): one chain, no branch in the graph


class TransformerLanguageModel(nn.Module):
    """model/lm.py:94-171: embed + posenc + post-norm GLU encoder layers (causal) + tied output."""

    def __init__(self, params):
        super().__init__()
        self.params = params
        self.model_type = 'transformer_lm'
        self.normalize_before = False
        self.smoothing = params['smoothing']
        self.vocab_size = params['vocab_size']
        self.num_blocks = params['num_blocks']
        self.embedding = nn.Embedding(self.vocab_size, params['d_model'])
        self.pos_embedding = PositionalEncoding(params['d_model'], 0.0)
        self.blocks = nn.ModuleList([
            TransformerEncoderLayer(params['n_heads'], params['d_model'], params['d_ff'], slf_attn_dropout=0.0,
                                    ffn_dropout=0.0, residual_dropout=params['residual_dropout'],
                                    normalize_before=False, concat_after=False, activation='glu')
            for _ in range(self.num_blocks)])
        self.output_project = nn.Linear(params['d_model'], self.vocab_size)
        if params['share_embedding']:
            self.output_project.weight = self.embedding.weight
        self.crit = LabelSmoothingLoss(size=self.vocab_size, smoothing=self.smoothing, padding_idx=PAD)

    def hidden(self, tokens):
        x = ops.embed_posenc(tokens.contiguous(), self.embedding.weight)
        for block in self.blocks:
            x, _ = block(x, None, causal=True)
        return x

    def logits(self, tokens):
        return ops.linear(self.hidden(tokens), self.output_project.weight, self.output_project.bias)

    def forward(self, inputs, targets):
        return self.crit(self.logits(inputs['inputs']), targets['targets']), None

    def predict(self, targets, last_frame=True):
        lg = self.logits(targets)
        if last_frame:
            return ops.log_softmax(lg[:, -1, :]).unsqueeze(1)
        return ops.log_softmax(lg)

    def set_epoch(self, epoch):
        pass


class RecurrentLanguageModel(nn.Module):
    """model/lm.py:33-91: nn.Embedding -> nn.LSTM(hidden, hidden, num_layers, batch_first) -> tied Linear, same constructor dict,
    attribute names and state_dict keys (`embedding.weight`, `rnn.weight_ih_l0` ...: a reference checkpoint loads strict).  On the hot
    path it is an INFERENCE component: the recognizers fuse its log-probabilities into the beam search (recognize/base.py:26-37), and
    the reference hands it the LAST token of every hypothesis with no carried state (recognize/speech2text.py:102-105 passes
    cache['lm'], which is never set) -- `logits_last`.  `predict` is the reference's general form (any prefix length, optional
    state).  The cell runs as two otr_linear_fwd GEMMs + otr_lstm_cell per layer and step; `self.rnn` only holds the parameters.
    forward() with a gradient wanted trains it (_train_forward: the otr_lstm_* step kernels and backpropagation through time);
    without one it evaluates the loss on the inference path above."""

    def __init__(self, params):
        super().__init__()
        self.params = params
        self.model_type = 'recurrent_lm'
        self.vocab_size = params['vocab_size']
        self.share_embedding = params['share_embedding']
        self.smoothing = params['smoothing']
        self.num_layers = params['num_layers']
        self.hidden_size = params['hidden_size']
        self.embedding = nn.Embedding(params['vocab_size'], params['hidden_size'])
        self.rnn = nn.LSTM(input_size=params['hidden_size'], hidden_size=params['hidden_size'], num_layers=params['num_layers'],
                           batch_first=True, dropout=params['dropout'], bidirectional=False)
        self.output_project = nn.Linear(params['hidden_size'], params['vocab_size'])
        if self.share_embedding:
            assert self.embedding.weight.size() == self.output_project.weight.size()
            self.output_project.weight = self.embedding.weight
        self.crit = LabelSmoothingLoss(size=self.vocab_size, smoothing=self.smoothing, padding_idx=PAD)

    def _layer_params(self, k):
        r = self.rnn
        return (getattr(r, 'weight_ih_l%d' % k), getattr(r, 'weight_hh_l%d' % k), getattr(r, 'bias_ih_l%d' % k), getattr(r, 'bias_hh_l%d' % k))

    def _step(self, x, h, c):
        """one time step through all layers; h / c: lists per layer (entries None = zero state)"""
        for k in range(self.num_layers):
            w_ih, w_hh, b_ih, b_hh = self._layer_params(k)
            ga = ops.linear(x, w_ih, b_ih)
            gb = ops.linear(h[k], w_hh, b_hh) if h[k] is not None else None          # W_hh . 0 = 0: the GEMM is skipped, b_hh stays
            h[k], c[k] = ops.lstm_cell(ga, gb, b_hh if gb is None else None, c[k])
            x = h[k]
        return x

    @torch.no_grad()
    def _run(self, tokens, hidden):
        B, T = tokens.shape
        nl = self.num_layers
        h = [None] * nl if hidden is None else [ops.attach_lp(hidden[0][k].contiguous().float(), hidden[0][k].to(ops.act_dtype()).contiguous())
                                                 if ops.is_half() else hidden[0][k].contiguous().float() for k in range(nl)]
        c = [None] * nl if hidden is None else [hidden[1][k].contiguous().float() for k in range(nl)]
        tokens = tokens.contiguous()
        outs = []
        for t in range(T):
            outs.append(self._step(ops.decode_lookup(tokens[:, t:t + 1], None, self.embedding.weight), h, c))
        y = torch.stack(outs, dim=1)
        return y, (torch.stack(h), torch.stack(c))

    def predict(self, pred, hidden=None):
        """model/lm.py:72-79: (log_probs [B, t, V], (h_n, c_n))"""
        y, hidden = self._run(pred, hidden)
        logits = ops.linear(y, self.output_project.weight, self.output_project.bias)
        return ops.log_softmax(logits), hidden

    @torch.no_grad()
    def logits_last(self, preds, pos=None, out=None):
        """un-normalised scores [R, V] of the token after preds[:, *pos] from the ZERO state: what the fused beam search adds at every
        step (recognize/base.py:35-36 with hidden = None); pos: device int32 scalar (cached search) or None = the last column"""
        if pos is None:
            preds, pos = preds[:, -1:], None
        x = ops.decode_lookup(preds, pos, self.embedding.weight)
        y = self._step(x, [None] * self.num_layers, [None] * self.num_layers)
        return _output(out, self.output_project, y)      # out: the _PaddedOutput of output_project ([R, rows8] logits) or None

    def forward(self, inputs, targets):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._train_forward(inputs['inputs'], targets['targets'])
        y, _ = self._run(inputs['inputs'], None)
        logits = ops.linear(y, self.output_project.weight, self.output_project.bias)
        return self.crit(logits, targets['targets']), None

    def _train_forward(self, tokens, target):
        """model/lm.py:63-70 with a backward pass: the sequence runs time-major (one contiguous [B, H] slice per step) through
        ops.embedding -> ops.lstm_layer per layer (nn.LSTM's dropout on the output of every layer but the last, off in eval()) ->
        output_project -> the label-smoothing loss.  Like the reference, nothing is packed: the LSTM runs over the PAD tail and only
        the loss masks it.  The fp16 loss scale registered by FusedAdam rides in the loss launch's gradient."""
        T = tokens.shape[1]
        x = ops.embedding(tokens.t(), self.embedding.weight)                 # [T, B, H]
        p = float(self.params['dropout'])
        for k in range(self.num_layers):
            if k:
                x = ops.dropout(x, p, self.training)
            x = ops.lstm_layer(x, *self._layer_params(k))
        logits = ops.linear(x, self.output_project.weight, self.output_project.bias)
        return self.crit.root(logits, target.t(), ops.loss_scale_of(self)), None

    def save_checkpoint(self, params, name):
        torch.save({'params': params, 'model': self.state_dict()}, name)

    def init_hidden_states(self, batch_size, device):
        return torch.zeros([self.num_layers, batch_size, self.hidden_size]).to(device)

    def set_epoch(self, epoch):
        pass


LanguageModel = {'rnn_lm': RecurrentLanguageModel, 'transformer_lm': TransformerLanguageModel}     # otrans/model/__init__.py:11-14


class Recognizer:
    """recognize/base.py:5-119."""

    def __init__(self, model, idx2unit=None, lm=None, lm_weight=None, ngpu=1):
        self.ngpu = ngpu
        self.model = model.eval()
        self.lm = lm.eval() if lm is not None else None
        self.idx2unit = idx2unit
        self.lm_weight = lm_weight

    def translate(self, seqs):
        results = []
        for seq in seqs:
            pred = []
            for i in seq:
                if int(i) == EOS:
                    break
                if int(i) == PAD:
                    continue
                pred.append(self.idx2unit[int(i)])
            results.append(' '.join(pred))
        return results

    def nbest_translate(self, nbest_preds):
        assert nbest_preds.dim() == 3
        results = []
        for b in range(nbest_preds.size(0)):
            nbest_list = []
            for n in range(nbest_preds.size(1)):
                pred = []
                for token in nbest_preds[b, n].tolist():
                    if token == EOS:
                        break
                    pred.append(self.idx2unit[token])
                nbest_list.append(' '.join(pred))
            results.append(nbest_list)
        return results


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size()) if t is not None else None


class _PaddedOutput:
    """The vocabulary projection of a decode step on ROW-PADDED operands (decoder/transformer.py:153, model/lm.py:60; the training
    path gets the same from dp.FlatDataParallel's padded slots): a 4234-row weight puts the rows of the [R, 4234] logits at odd
    addresses and the product on the generic loaders -- 87 + 41 us of a 0.6 ms decode step for the decoder's and the LM's output layers
    (rocprofv3, profiles/r05_decode_kernels.txt).  Here: a 16-bit copy of the weight with the rows padded to a multiple of 8 (zeros),
    the bias likewise, the logits come out as [R, rows8] and otr_beam_topk reads them through their leading dimension.  Built once per
    (weights' version, pointer) fingerprint by the owners below: a changed checkpoint rebuilds it."""

    def __init__(self, weight, bias):
        N, K = weight.shape
        self.N, self.N8 = N, (N + 7) // 8 * 8
        hdt = ops.half_dtype()
        self.w = torch.zeros((self.N8, K), dtype=hdt, device=weight.device)
        self.w[:N].copy_(weight.detach())
        self.b = None
        if bias is not None:
            self.b = torch.zeros((self.N8,), dtype=torch.float32, device=weight.device)
            self.b[:N].copy_(bias.detach())

    def __call__(self, x):
        """x [R, K] fp32 with its 16-bit twin (or 16-bit) -> logits [R, N8] fp32 (columns >= N are zero-weight products: ignored)"""
        x16 = ops.lp_of(x)
        x2 = (x16 if x16 is not None else x).reshape(-1, self.w.shape[1])
        if x2.dtype != self.w.dtype:
            x2 = x2.to(self.w.dtype)
        return ops.linear_fwd_raw(x2.contiguous(), self.w, self.b, torch.float32)


def _padded_output(weight, bias):
    """a _PaddedOutput where it pays (16-bit mode, CUDA, output width not a multiple of 8), else None"""
    if ops.is_half() and weight.is_cuda and weight.dim() == 2 and weight.shape[0] % 8 != 0 and weight.shape[1] % 8 == 0:
        return _PaddedOutput(weight, bias)
    return None


def _output(padded, layer, x):
    """the vocabulary projection of a decode step: the _PaddedOutput of `layer` where there is one, else ops.linear"""
    return padded(x) if padded is not None else ops.linear(x, layer.weight, layer.bias)


class _FusedChain:
    """One post-norm stack's position in a chain of fused decode launches (csrc/declayer.hip): its residual rows, the descriptor of
    the add + LayerNorm the NEXT launch finishes in its prologue (ops._dec_ln), and `keep`, the tensors that descriptor points at --
    it holds raw pointers, so they stay alive until that launch is queued.  The stages of a layer: [LayerNorm of the layer below +
    q|k|v + cached self-attention + output projection] (self_item), for a decoder layer (kvs given) [LayerNorm + q + cross-attention
    over the utterance memory + output projection] (cross: the beam hypotheses of an utterance are the query rows of ONE attention
    problem, exactly the training launch with L = beam), [LayerNorm + w_1 + GLU + w_2] cut into slices(F) hidden slices (ffn_item).
    Each stage leaves its output in slabs that `close` turns into the next descriptor.  CachedBeamState._walk issues the launches."""

    def __init__(self, st, cur, x, blocks, caches, kvs, slices):
        self.st, self.cur, self.blocks, self.caches, self.kvs, self.slices, self.li = st, cur, blocks, caches, kvs, slices, 0
        x16 = ops.lp_of(x)
        self.yres, self.keep = x.reshape(st.R, 256), [x, x16]
        self.ln = ops._dec_ln(None, x16.reshape(st.R, 256), None, 0)       # the rows are normalised already: nothing to finish

    def _h16(self, *shape):
        return torch.empty(shape, dtype=ops.half_dtype(), device=self.yres.device)

    def close(self, slabs, bias, norm):
        """the residual add + LayerNorm that closes a sub-layer whose output is the partial sums `slabs`: left to the next launch"""
        y, y16 = torch.empty_like(self.yres), self._h16(*self.yres.shape)
        self.ln = ops._dec_ln(self.yres, None, slabs, slabs.shape[0], bias, norm.weight, norm.bias, None, 0.0, norm.eps, 0, y, y16)
        self.keep = [self.yres, slabs, y, y16]
        self.yres, self.y16 = y, y16

    def self_item(self):
        blk, st = self.blocks[self.li], self.st
        a, slabs = blk.slf_attn, self._h16(4, st.R, 256)
        it = L.DecSelfStep()
        it.ln, it.R = self.ln, st.R
        it.wqkv_pack, it.bqkv = ops.lin_packs(a.qvk_proj.weight)[0].data_ptr(), a.qvk_proj.bias.data_ptr()
        it.wo_pack = ops.lin_packs(a.output_proj.weight)[0].data_ptr()
        it.kcache, it.vcache = self.caches[self.li][0].data_ptr(), self.caches[self.li][1].data_ptr()
        it.anc, it.pos, it.maxlen, it.slabs = st.anc[self.cur].data_ptr(), st.pos[self.cur].data_ptr(), st.maxlen, slabs.data_ptr()
        self.closing = (slabs, a.output_proj.bias, blk.norm1)
        return it

    def cross(self, lib, stream):
        if self.kvs is None:
            return
        blk, kv, st = self.blocks[self.li], self.kvs[self.li], self.st
        ca, R, beam = blk.src_attn, st.R, st.rec.beam_width
        slB, q16, ctx2 = self._h16(4, R, 256), self._h16(R, 256), self._h16(R, 256)
        lse2 = torch.empty((st.b, 4, beam), dtype=torch.float32, device=self.yres.device)
        W = kv.shape[2]
        L.check(lib.otr_dec_cross_fwd(C.byref(self.ln), st.b, beam, ops._p(ops.lin_packs(ca.q_proj.weight)[0]), ops._p(ca.q_proj.bias),
                                      ops._p(ops.lin_packs(ca.output_proj.weight)[0]), ops._p(kv), st.Tm * W, W, 0, W // 2,
                                      ops._p(st.mem_mask), st.Tm, ops._p(q16), ops._p(ctx2), ops._p(lse2), ops._p(slB), stream),
                'otr_dec_cross_fwd')
        self.close(slB, ca.output_proj.bias, blk.norm2)

    def ffn_item(self):
        blk, R = self.blocks[self.li], self.st.R
        ff = blk.feed_forward
        F = ff.w_2.weight.shape[1]
        S = self.slices(F)
        packs, slabs = ops.ffn_packs(ff.w_1.weight, ff.w_2.weight), self._h16(S, R, 256)
        it = L.DecFfnFwd()
        it.ln, it.R = self.ln, R
        it.w1_pack, it.b1, it.w2_pack = packs[0].data_ptr(), ff.w_1.bias.data_ptr(), packs[1].data_ptr()
        it.F, it.S, it.slabs, it.hsave = F, S, slabs.data_ptr(), None
        self.closing = (slabs, ff.w_2.bias, blk.norm3 if self.kvs is not None else blk.norm2)
        return it

    def out(self):
        return ops.attach_lp(self.yres, self.y16)


def _issue(lib, name, items, stream):
    """one launch of a stage: `name`_pair on the items of two chains, else the single entry on the one item (its fields after `ln`
    are the single entry's arguments, in order)"""
    if len(items) == 2:
        L.check(getattr(lib, name + '_pair')(C.byref(items[0]), C.byref(items[1]), stream), name + '_pair')
    else:
        it = items[0]
        L.check(getattr(lib, name)(C.byref(it.ln), *[getattr(it, f) for f, _ in it._fields_[1:]], stream), name)


class _JointCTC:
    """Device state of the joint CTC/attention search (include/otrans_hip.h, csrc/ctcscore.hip) for R = B * beam hypotheses over T'
    frames: the CTC head's log-probs and lengths, the pre-beam candidates, the prefix states double-buffered per ping-pong phase like
    preds / scores (a step reading phase cur writes phase cur ^ 1 only), the survivors' state slots and the top-beam's slots."""

    def __init__(self, B, T, V, K, beam, dev):
        R = B * beam
        self.K = K
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)    # noqa: E731
        self.lp = new((B, T, V), torch.float32)
        self.lengths = new((B,), torch.int32)
        self.cand_s, self.cand_i = new((R, K), torch.float32), new((R, K), torch.int32)
        self.state = [(new((R * K, T), torch.float32), new((R * K, T), torch.float32), new((R * K,), torch.float32)) for _ in range(2)]
        self.jsrc = [new((R,), torch.int32) for _ in range(2)]
        self.k_src = new((R, beam), torch.int32)

    def load(self, log_probs, lengths):
        self.lp.copy_(log_probs)
        self.lengths.copy_(lengths.reshape(-1))


class _BeamState:
    """The beams of one search over R = B * beam hypotheses, for both decode loops: ping-pong prefixes / scores / finished flags (a
    step reads phase cur and writes phase cur ^ 1 only), the per-row top-beam the scoring hands to the prune, the finished counter and,
    where the recognizer asks for them, the joint search's state and the pinned n-gram LM / phrase table with the plain search's pre-beam
    candidates.
    cached: the counter is [finished hypotheses, the prune kernel's arrival word] per phase, as otr_beam_prune_cached takes it -- the
    count of a step stays readable while the next step runs (CachedBeamState.run) --, else the one count of otr_beam_prune."""

    def __init__(self, rec, b, Tm, dev, cached):
        beam = rec.beam_width
        R = b * beam
        self.rec, self.b, self.Tm, self.dev, self.beam, self.R = rec, b, Tm, dev, beam, R
        self.V = rec.model.decoder.output_layer.weight.shape[0]
        self.ldp = rec.max_len + 2
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)    # noqa: E731
        self.preds = [new((R, self.ldp), torch.long) for _ in range(2)]
        self.scores = [new((R,), torch.float32) for _ in range(2)]
        self.flags = [new((R,), torch.uint8) for _ in range(2)]
        self.k_score = new((R, beam), torch.float32)
        self.k_idx = new((R, beam), torch.long)
        self.n_fin = new((2, 2) if cached else (1,), torch.int32)
        self.score0 = torch.tensor([0.0] + [-float('inf')] * (beam - 1), device=dev).repeat([b]).contiguous()
        self.joint = _JointCTC(b, Tm, self.V, rec.ctc_beam, beam, dev) if rec.joint_ctc else None
        self.ngram = rec.ngram_lm.to(dev) if rec.ngram_lm is not None else None     # pinned: a cached state's key holds its table's address
        self.bias = rec.bias.to(dev) if rec.bias is not None else None              # pinned likewise
        self.cand = None
        if (self.ngram is not None or self.bias is not None) and self.joint is None:
            # the plain search with an n-gram or phrases: pre-beam + addend(s) + select, no full top-k
            K = rec.ngram_beam if self.ngram is not None else rec.bias_beam
            self.cand = (new((R, K), torch.float32), new((R, K), torch.int32))

    def reset(self):
        """the start of a search in phase 0: BOS alone in every prefix, one live hypothesis per utterance, nothing finished"""
        self.preds[0].fill_(EOS)
        self.preds[0][:, 0] = BOS
        self.scores[0].copy_(self.score0)
        self.flags[0].zero_()
        self.n_fin.zero_()       # incl. the prune kernel's arrival word: a launch aborted mid-step would leave it poisoned for every later batch

    def advance(self, logits, lm_logits, cur, t=0, pos=None, anc=None, maxlen=0):
        """The scoring tail of one step (recognize/speech2text.py:102-146), reading phase cur, writing phase cur ^ 1.  logits and
        lm_logits (or None): the next-token scores as 2-D views [R, >= V] of any row stride.  The prefixes have t columns (the
        re-forward loop's host step), or pos[cur] + 1 where the cached loop gives its per-phase device positions `pos` with the
        ancestor tables `anc` of width maxlen."""
        rec, lib, nxt, j = self.rec, L.load(), cur ^ 1, self.joint
        V, beam, lm_weight = self.V, self.beam, float(rec.lm_weight or 0.0)
        preds, scores, flags = self.preds, self.scores, self.flags
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p_cur = pos[cur] if pos is not None else None
        if j is not None:                                 # pre-beam top-K' (+ the n-gram's addend, in place) + CTC prefix scores + joint top-beam
            lam = float(rec.ctc_weight)
            ops.joint_prebeam(logits, lm_logits, 1.0 - lam, lm_weight, j.K, V, j.cand_s, j.cand_i)
            if self.ngram is not None:                    # the prefix score ranks by counting, in any order
                ops.ngram_score_candidates(self.ngram, preds[cur], j.cand_i, j.cand_s, rec.alpha, rec.beta, EOS, t=t, pos=p_cur,
                                           flags=flags[cur], cand_out=j.cand_s)
            if self.bias is not None:                     # behind the n-gram's addend, in place as well
                ops.bias_score_candidates(self.bias, preds[cur], j.cand_i, j.cand_s, EOS, t=t, pos=p_cur, flags=flags[cur],
                                          cand_out=j.cand_s)
            ops.ctc_prefix_score(j.lp, j.lengths, j.cand_i, preds[cur], t, beam, rec.model.assistor.blank, EOS, j.jsrc[cur], j.state[cur],
                                 j.state[nxt], pos=p_cur, cand_score=j.cand_s, ctc_weight=lam, beam=beam, flags=flags[cur],
                                 k_score=self.k_score, k_idx=self.k_idx, k_src=j.k_src)
        elif self.cand is not None:                       # pre-beam + addend(s) + select in otr_beam_topk's place: the last scorer selects
            select = dict(beam=beam, k_score=self.k_score, k_idx=self.k_idx)
            ops.joint_prebeam(logits, lm_logits, 1.0, lm_weight, self.cand[0].shape[1], V, *self.cand)
            if self.ngram is not None:
                ops.ngram_score_candidates(self.ngram, preds[cur], self.cand[1], self.cand[0], rec.alpha, rec.beta, EOS, t=t, pos=p_cur,
                                           flags=flags[cur], cand_out=self.cand[0], **({} if self.bias is not None else select))
            if self.bias is not None:
                ops.bias_score_candidates(self.bias, preds[cur], self.cand[1], self.cand[0], EOS, t=t, pos=p_cur, flags=flags[cur],
                                          cand_out=self.cand[0], **select)
        else:
            L.check(lib.otr_beam_topk(_ptr(logits), logits.stride(0), _ptr(lm_logits), lm_logits.stride(0) if lm_logits is not None else V,
                                      lm_weight, self.R, V, beam, _ptr(self.k_score), _ptr(self.k_idx), stream), 'otr_beam_topk')
        # the prune: {host t, device pos} x {plain, joint}
        args = [_ptr(self.k_score), _ptr(self.k_idx), _ptr(scores[cur]), _ptr(flags[cur]), _ptr(preds[cur]), self.ldp, self.b, beam]
        out = [_ptr(scores[nxt]), _ptr(flags[nxt]), _ptr(preds[nxt])]
        if pos is None:
            args += [t, EOS] + out + [_ptr(self.n_fin)]
        else:
            args += [EOS, _ptr(pos[cur]), _ptr(pos[nxt]), _ptr(anc[cur]), _ptr(anc[nxt]), maxlen] + out + [_ptr(self.n_fin[nxt])]
        if j is not None:
            args += [_ptr(j.k_src), _ptr(j.jsrc[nxt])]
        if pos is None and j is None:
            L.check(lib.otr_beam_prune(*args, stream), 'otr_beam_prune')
        elif pos is None:
            L.check(lib.otr_beam_prune_joint(*args, stream), 'otr_beam_prune_joint')
        elif j is None:
            L.check(lib.otr_beam_prune_cached(*args, stream), 'otr_beam_prune_cached')
        else:
            L.check(lib.otr_beam_prune_cached_joint(*args, stream), 'otr_beam_prune_cached_joint')


def _lm_recurrent(lm):
    """True for the RecurrentLanguageModel, False for the Transformer LM, None for any other model_type (the step loops run such an LM
    like the Transformer LM, rescore=True refuses it).  The one reader of model_type."""
    return {'recurrent_lm': True, 'transformer_lm': False}.get(getattr(lm, 'model_type', ''))


def _lm_logits(lm, tokens, pos=None, out=None, hidden=None, every=False):
    """The LM's un-normalised scores of the next token (None without an LM) after the last column of the prefixes `tokens` [R, t] -- a
    2-D view [R, >= V] of any row stride -- or, with `every`, after each column (the rescore pass over ys_in).  The cached loop
    passes preds with its device position `pos`, the _PaddedOutput `out` and `hidden`, which gives the Transformer LM's rows of that
    position from its K/V caches.  The recurrent LM scores the last token alone from the ZERO state (recognize/base.py:35-36)."""
    if lm is None:
        return None
    if _lm_recurrent(lm):
        return lm.logits_last(tokens.reshape(-1, 1) if every else tokens, pos, out=out)
    lg = _output(out, lm.output_project, hidden() if hidden is not None else lm.hidden(tokens))
    return lg if every or hidden is not None else lg[:, -1]


def _vocab_limit(who, V):
    if V > ops.JOINT_MAX_V:
        raise ValueError('%s: vocabulary %d > %d' % (who, V, ops.JOINT_MAX_V))


def _prebeam_limits(who, name, beam_width, K, V):
    """the pre-beam's limits (include/otrans_hip.h), refused in the constructor; returns the pre-beam width `name` (K, or ESPnet's
    default min(V, int(1.5 * beam_width)))"""
    if not 1 <= beam_width <= ops.JOINT_MAX_BEAM:
        raise ValueError('%s: beam_width=%d must be in [1, %d]' % (who, beam_width, ops.JOINT_MAX_BEAM))
    _vocab_limit(who, V)
    K = int(K) if K is not None else min(V, int(1.5 * beam_width))
    if not beam_width <= K <= min(V, ops.JOINT_MAX_K):
        raise ValueError('%s: %s=%d must be in [beam_width=%d, min(V=%d, %d)]' % (who, name, K, beam_width, V, ops.JOINT_MAX_K))
    return K


def _mbr_args(who, mbr, mbr_scale, beam_width):
    """(mbr, mbr_scale) of a recognizer's constructor, checked"""
    mbr_scale = float(mbr_scale)
    if not math.isfinite(mbr_scale):
        raise ValueError('%s: mbr_scale=%r must be finite' % (who, mbr_scale))
    if mbr and not 1 <= beam_width <= ops.EDIT_MAX_NBEST:
        raise ValueError('%s: mbr=True takes the consensus of the whole beam: beam_width=%d, 1 .. %d supported'
                         % (who, beam_width, ops.EDIT_MAX_NBEST))
    return bool(mbr), mbr_scale


def _consensus_nbest(tokens, lengths, scores, scale, mbr, n, eos, follow=None):
    """The consensus of a final beam (tokens [B, W, L], lengths [B, W], scores [B, W], best score first) and the n-best it leaves:
    ordered by ascending risk where `mbr` (a stable sort: ties keep the higher score, then the lower rank; dead slots, of risk +inf,
    last), as it stands otherwise.  -> (tokens [B, n, L], lengths [B, n], scores [B, n], conf f32 [B, L] and post f32 [B] of the
    1-best).  Only the first ops.NBEST_MAX_LEN columns go into the consensus: a longer hypothesis is a dead slot there.  No host
    synchronisation.  follow: a tensor [B, W, L] that belongs to the tokens (the transducer's frames); it is cut and permuted as
    they are and returned as a sixth element."""
    L_ = tokens.size(-1)
    post, risk, _, conf = ops.nbest_consensus(tokens[:, :, :ops.NBEST_MAX_LEN], lengths, scores, scale=scale, eos=eos)
    if conf.size(-1) < L_:
        conf = torch.nn.functional.pad(conf, (0, L_ - conf.size(-1)))
    if not mbr:
        out = (tokens[:, :n], lengths[:, :n], scores[:, :n], conf[:, 0], post[:, 0])
        return out if follow is None else out + (follow[:, :n],)
    order = torch.sort(risk, dim=-1, stable=True)[1][:, :n]
    first = order[:, :1]
    wide = order.unsqueeze(-1).expand(-1, -1, L_)
    out = (torch.gather(tokens, 1, wide), torch.gather(lengths, 1, order), torch.gather(scores, 1, order),
           torch.gather(conf, 1, first.unsqueeze(-1).expand(-1, -1, L_))[:, 0], torch.gather(post, 1, first)[:, 0])
    return out if follow is None else out + (torch.gather(follow, 1, wide),)


class SpeechToTextRecognizer(Recognizer):
    """recognize/speech2text.py:6-153.
    joint_ctc=False (the default, as in the reference): attention decoder (+ LM shallow fusion) only; ctc_weight is accepted and unused.
    joint_ctc=True: hybrid CTC/attention decoding (Watanabe et al. 2017, Algorithm 2; ESPnet's CTCPrefixScore) with the model's CTC
    head (model.assistor, built when the model was trained with ctc_weight > 0): per hypothesis the ctc_beam tokens of highest
    (1 - ctc_weight) * att + lm_weight * lm are scored (1 - ctc_weight) * att + lm_weight * lm + ctc_weight * (psi(h) - psi(g)), psi the
    CTC prefix score, and the beam best of them go to the usual prune.  The score of a hypothesis that ended in EOS is then
    (1 - ctc_weight) log P_att + ctc_weight log P_ctc + lm_weight log P_lm.  ctc_beam defaults to min(V, int(1.5 * beam_width)) as in
    ESPnet.  Both decode loops; under apply_cache the joint step is part of the captured graph.  include/otrans_hip.h states the
    semantics and the limits (beam_width <= 16, beam_width <= ctc_beam <= min(V, 32), T' <= 2048).
    rescore=True: two-pass decoding, no step loop.  The beam_width best hypotheses of the CTC prefix beam search (cutoff_top_n candidates
    per frame, ops.ctc_prefix_beam_search) are scored by the attention decoder -- and the LM -- in ONE teacher-forced pass each and
    re-ranked by (1 - ctc_weight) att + ctc_weight ctc + lm_weight lm, ctc being the beam's own score (include/otrans_hip.h
    otr_rescore_*, csrc/rescore.hip).  A hypothesis longer than max_len - 1 tokens is not rescored and sorts last.  Limits:
    nbest <= beam_width <= 32, V <= 8192; not together with joint_ctc or apply_cache.
    ngram_lm: None, or an ngram.NGramLM over the decoder's V units (NGramLM.from_arpa).  In the step loops every pre-beam candidate c of
    hypothesis g then gains alpha * ln P_ng(c | <s> g) + beta (EOS: scored as </s>, no beta) before it is ranked (include/otrans_hip.h
    otr_ngram_score_cands): in the joint search the ctc_beam candidates, in the plain search the ngram_beam tokens of highest att + lm
    (ngram_beam defaults to min(V, int(1.5 * beam_width)); limits beam_width <= 16, beam_width <= ngram_beam <= min(V, 32), V <= 8192),
    which replace otr_beam_topk's full-vocabulary top-k.  With rescore=True the n-gram is fused into the first pass
    (ops.ctc_prefix_beam_search_lm) and the second pass adds the hypothesis's n-gram score, computed afresh with its </s> term
    (otr_ngram_score_seqs), to the total.  alpha / beta default as in CTCRecognizer.  A path is not loaded here (build_recognizer does).
    bias: None, or a bias.PhraseBias over the decoder's V units (phrase biasing, "hotwords"; include/otrans_hip.h otr_bias_score_cands
    states the rule).  In the step loops every pre-beam candidate c of hypothesis g gains psi_minus(state(g c)) - psi(state(g)) -- the
    per-token weight while g c spells on at a phrase, the refund of an unfinished match where it stops -- behind the n-gram's addend, if
    any: in the joint search on the ctc_beam candidates, in the plain search on the K' tokens of highest att + lm, K' = ngram_beam
    where an n-gram LM is given (a bias_beam that differs from it is refused), else bias_beam (default min(V, int(1.5 * beam_width)),
    the pre-beam's limits).  ONLY pre-beam candidates are boosted: a phrase continuation the pre-beam dropped is not brought back;
    raise K' (up to 32) for deeper reach.  With rescore=True the second pass adds the phrase score of each hypothesis
    (otr_bias_score_seqs; res['bias']) to the total, beside the n-gram's.  By default (bias_first_pass=False) the first pass (the CTC
    prefix beam search) is NOT biased, so phrases re-rank the n-best and no more.  bias_first_pass=True makes the first pass the
    phrase-biased search (ops.ctc_prefix_beam_search_bias, with the n-gram too where one is given): a phrase the acoustic model ranks
    below the beam can then reach the second pass.  The acoustic term becomes scores - lm_scores - bias_scores of that search and the
    total of a hypothesis keeps its formula; only which hypotheses are rescored changes.  bias_first_pass=True needs rescore=True and
    a bias, and none of the phrases may hold the CTC head's blank.
    mbr=True: minimum Bayes risk selection, in every mode.  The whole final beam (not only the nbest kept) is taken as a posterior,
    softmax(mbr_scale * score), every hypothesis gets its expected edit distance against the others under it (ops.nbest_consensus,
    include/otrans_hip.h otr_nbest_consensus) and the n-best is ordered by ascending risk, ties to the higher score, then the lower
    rank, before nbest is cut; the scores returned are still the search's.  beam_width <= 32; a hypothesis of more than
    ops.NBEST_MAX_LEN tokens is left out of the consensus and sorts last.  recognize_with_confidence gives the 1-best's tokens the
    posterior mass that agrees with them, with or without mbr."""

    def __init__(self, model, lm=None, lm_weight=0.1, ctc_weight=0.0, beam_width=5, nbest=1, max_len=50,
                 idx2unit=None, penalty=0, lamda=5, ngpu=1, apply_cache=False, joint_ctc=False, ctc_beam=None, rescore=False,
                 cutoff_top_n=40, ngram_lm=None, alpha=0.1, beta=0.0, ngram_beam=None, bias=None, bias_beam=None,
                 bias_first_pass=False, mbr=False, mbr_scale=1.0):
        super().__init__(model, idx2unit, lm, lm_weight, ngpu)
        self.mbr, self.mbr_scale = _mbr_args('SpeechToTextRecognizer', mbr, mbr_scale, beam_width)
        if bias_first_pass and (not rescore or bias is None):
            raise ValueError('bias_first_pass=True biases the first pass of the two-pass decode: it needs rescore=True and bias=...')
        self.bias_first_pass = bool(bias_first_pass)
        if ngram_lm is not None and not isinstance(ngram_lm, NGramLM):
            raise NotImplementedError('SpeechToTextRecognizer: ngram_lm must be an NGramLM, not %s: load the ARPA file with '
                                      'NGramLM.from_arpa(path, idx2unit) (KenLM binaries are not read)' % type(ngram_lm).__name__)
        self.ngram_lm, self.alpha, self.beta, self.ngram_beam = ngram_lm, float(alpha), float(beta), None
        if bias is not None and not isinstance(bias, PhraseBias):
            raise TypeError('SpeechToTextRecognizer: bias must be a PhraseBias, not %s: build one with PhraseBias(phrases, vocab_size) or '
                            'PhraseBias.from_texts(lines, idx2unit)' % type(bias).__name__)
        self.bias, self.bias_beam = bias, None
        self.rescore, self.cutoff_top_n = bool(rescore), int(cutoff_top_n)
        if self.rescore:
            if joint_ctc or apply_cache:
                raise ValueError('rescore=True replaces the step loop: not together with %s' % ('joint_ctc=True' if joint_ctc else 'apply_cache=True'))
            if getattr(model, 'assistor', None) is None:
                raise ValueError('rescore=True needs the model\'s CTC head (model.assistor): build the model with ctc_weight > 0')
            _rescore_check('rescore=True', beam_width, model.decoder.output_layer.weight.shape[0], nbest, ctc_weight)
            if max_len < 1 or self.cutoff_top_n < 1:
                raise ValueError('rescore=True: max_len=%d and cutoff_top_n=%d must be >= 1' % (max_len, self.cutoff_top_n))
            if lm is not None and _lm_recurrent(lm) is None:
                raise ValueError('rescore=True: the language model %r cannot be scored teacher-forced here (TransformerLanguageModel and '
                                 'RecurrentLanguageModel can)' % type(lm).__name__)
            self._rescore_out = None
        self.beam_width, self.max_len, self.nbest = beam_width, max_len, nbest
        self.penalty, self.lamda, self.ctc_weight, self.lm_weight = penalty, lamda, ctc_weight, lm_weight
        self.joint_ctc, self.ctc_beam = bool(joint_ctc), None
        V = model.decoder.output_layer.weight.shape[0] if self.joint_ctc or ngram_lm is not None or bias is not None else None
        if self.joint_ctc:
            if getattr(model, 'assistor', None) is None:
                raise ValueError('joint_ctc=True needs the model\'s CTC head (model.assistor): build the model with ctc_weight > 0')
            if not 0.0 <= float(ctc_weight) <= 1.0:
                raise ValueError('joint_ctc=True: ctc_weight=%r must be in [0, 1]' % (ctc_weight,))
            self.ctc_beam = _prebeam_limits('joint_ctc=True', 'ctc_beam', beam_width, ctc_beam, V)
        if ngram_lm is not None:
            if ngram_lm.vocab_size != V:
                raise ValueError('ngram_lm: the n-gram LM was loaded for %d units, the decoder has V=%d' % (ngram_lm.vocab_size, V))
            _vocab_limit('ngram_lm', V)
            if not self.rescore and not self.joint_ctc:       # the plain search pre-beams too (the joint search's limits are checked above)
                self.ngram_beam = _prebeam_limits('ngram_lm', 'ngram_beam', beam_width, ngram_beam, V)
        if bias is not None:
            if bias.vocab_size != V:
                raise ValueError('bias: the phrases were built for %d units, the decoder has V=%d' % (bias.vocab_size, V))
            _vocab_limit('bias', V)
            if not self.rescore and not self.joint_ctc:       # the plain search pre-beams: with the n-gram's K' where there is one
                if self.ngram_beam is not None:
                    if bias_beam is not None and int(bias_beam) != self.ngram_beam:
                        raise ValueError('bias: bias_beam=%d differs from ngram_beam=%d: the two scorers share one pre-beam'
                                         % (bias_beam, self.ngram_beam))
                    self.bias_beam = self.ngram_beam
                else:
                    self.bias_beam = _prebeam_limits('bias', 'bias_beam', beam_width, bias_beam, V)
        self.attn_weights = {}
        self.apply_cache = bool(apply_cache)
        self.use_hipgraph = True
        self._cached_states = {}
        self.trace = None       # test hook: a list collects (prefixes [B*beam, step+1], cumulative scores [B*beam]) after every step

    def encode(self, inputs, inputs_mask, cache=None):
        x, mask, fe_cache = self.model.frontend.inference(inputs, inputs_mask, None)
        memory, memory_mask, attn = self.model.encoder(x, mask)
        return memory, memory_mask, {'frontend': fe_cache}, attn

    def _ctc_head(self, memory, memory_mask):
        """the CTC head's f32 log-probs [B, T', V] and int32 lengths [B] for the joint search; T' is refused before the first launch"""
        if memory.size(1) > ops.JOINT_MAX_T:
            raise ValueError('joint_ctc=True: T\'=%d encoder frames > %d' % (memory.size(1), ops.JOINT_MAX_T))
        log_probs, length = self.model.assistor.inference(memory, memory_mask)
        return log_probs.float().contiguous(), length.to(torch.int32).contiguous()

    def _nbest(self, scores, preds, steps, b):
        """n-best selection on the host: B*beam scalars (speech2text.py:70-93)"""
        beam = self.beam_width
        scores_h = scores.cpu().view(b, beam)
        preds_h = preds[:, :steps + 1].cpu().view(b, beam, -1)
        lengths = torch.sum(torch.ne(preds_h, EOS).float(), dim=-1)
        if self.penalty:
            scores_h = scores_h / torch.pow((self.lamda + lengths) / (self.lamda + 1), self.penalty)
        sorted_scores, offset = torch.sort(scores_h, dim=-1, descending=True)
        sorted_preds = torch.gather(preds_h, 1, offset.unsqueeze(-1).expand_as(preds_h))
        nbest_preds = sorted_preds[:, :min(beam, self.nbest), 1:]
        nbest_scores = sorted_scores[:, :min(beam, self.nbest)]
        return self.nbest_translate(nbest_preds), nbest_scores

    def _nbest_device(self, scores, preds, steps, b, n=None):
        """_nbest's selection with torch ops on the device, no copy to the host: (tokens int64 [B, n, steps] without BOS, lengths int32
        [B, n]: a hypothesis ends before its first EOS, scores f32 [B, n]).  Equal scores may sort in another order than on the host.
        Without a length penalty the scores are the search's own, bit for bit _nbest's; with one the pow and the division run on
        the device here and on the host there, so they agree to float32 rounding only."""
        beam = self.beam_width
        scores_d = scores.view(b, beam)
        preds_d = preds[:, :steps + 1].reshape(b, beam, -1)
        if self.penalty:
            lengths = torch.sum(torch.ne(preds_d, EOS).float(), dim=-1)
            scores_d = scores_d / torch.pow((self.lamda + lengths) / (self.lamda + 1), self.penalty)
        sorted_scores, offset = torch.sort(scores_d, dim=-1, descending=True)
        n = min(beam, self.nbest) if n is None else n
        tokens = torch.gather(preds_d, 1, offset[:, :n].unsqueeze(-1).expand(b, n, preds_d.size(-1)))[:, :, 1:].contiguous()
        is_eos = torch.eq(tokens, EOS)
        first = torch.where(is_eos.any(-1), is_eos.to(torch.int32).argmax(-1), torch.full_like(offset[:, :n], tokens.size(-1)))
        return tokens, first.to(torch.int32), sorted_scores[:, :n].contiguous()

    @torch.no_grad()
    def recognize_tokens(self, inputs, inputs_mask):
        """recognize() without the host: the n-best as device tensors (tokens int64 [B, n, L] without BOS, lengths int32 [B, n], scores
        f32 [B, n]), best first, for ops.edit_distance / evaluate.ErrorRateMeter.  The same searches and the same selection as
        recognize(): nbest_translate(tokens) gives its strings (it stops at the first EOS, which is where a length ends).  On the re-forward and cached
        paths a hypothesis ends before its first EOS; on the rescore path the search's < 0 padding marks the end.  With mbr=True the
        n-best is in ascending order of risk."""
        if self.mbr:
            return self.recognize_tokens_with_confidence(inputs, inputs_mask)[:3]
        return self._beam_device(inputs, inputs_mask, min(self.beam_width, self.nbest))

    def _beam_device(self, inputs, inputs_mask, n):
        """the n best-scoring hypotheses of the final beam as recognize_tokens returns them; n = beam_width: the whole beam"""
        if self.rescore:
            res = self._rescore(inputs, inputs_mask, nbest=n)
            tok = res['tokens']
            return tok.masked_fill(tok < 0, EOS), torch.sum(tok >= 0, dim=-1, dtype=torch.int32), res['scores']
        search = self._search_cached if self.apply_cache else self._search
        return self._nbest_device(*search(inputs, inputs_mask), n=n)

    @torch.no_grad()
    def recognize_tokens_with_confidence(self, inputs, inputs_mask):
        """recognize_tokens() plus the consensus of the whole final beam (ops.nbest_consensus at mbr_scale), all on the device: (tokens,
        lengths, scores of the n-best -- in ascending order of risk with mbr=True, by score otherwise --, conf f32 [B, L]: per token
        of the 1-best the posterior mass of the hypotheses whose alignment matches it, post f32 [B]: the 1-best's own posterior)."""
        return _consensus_nbest(*self._beam_device(inputs, inputs_mask, self.beam_width), self.mbr_scale, self.mbr,
                                min(self.beam_width, self.nbest), EOS)

    @torch.no_grad()
    def recognize_with_confidence(self, inputs, inputs_mask):
        """recognize() with token confidences: (texts: recognize()'s n-best strings, confidences: per utterance [(unit, confidence), ...]
        for the 1-best, its units read in order being the words of its text, utt_posterior: the 1-best's posterior, a host tensor [B])"""
        tokens, lengths, _, conf, post = self.recognize_tokens_with_confidence(inputs, inputs_mask)
        tok, n, conf = tokens.cpu(), lengths.cpu(), conf.cpu()
        texts = self.nbest_translate(torch.cat((tok, torch.full_like(tok[:, :, :1], EOS)), dim=-1))
        confidences = [[(self.idx2unit[int(tok[b, 0, k])], float(conf[b, k])) for k in range(int(n[b, 0]))] for b in range(tok.size(0))]
        return texts, confidences, post.cpu()

    @torch.no_grad()
    def recognize_cached(self, inputs, inputs_mask):
        return self._nbest(*self._search_cached(inputs, inputs_mask))

    @torch.no_grad()
    def _search_cached(self, inputs, inputs_mask):
        """the cached beam search: (scores [B*beam], prefixes [B*beam, >= steps + 1] with BOS, steps, B) on the device"""
        memory, memory_mask, _, _ = self.encode(inputs, inputs_mask)
        b, t, _ = memory.size()
        head = self._ctc_head(memory, memory_mask) if self.joint_ctc else None
        # the captured graphs bake in the device pointers of the stand-alone 16-bit weight shadows (ops.weight_lp caches a
        # cast per parameter version): a checkpoint loaded into the same modules, averaging, ... re-allocates them, so the
        # weights' (version, pointer) fingerprint is part of the key -- stale graphs are dropped, never replayed
        fp = 0
        for mod in (self.model.decoder, self.lm, self.model.assistor if self.joint_ctc else None):
            if mod is not None:
                for p_ in mod.parameters():
                    fp = (fp * 1000003 + p_._version * 31 + p_.data_ptr()) & 0xFFFFFFFFFFFF
        key = (b, t, self.beam_width, self.max_len, ops.get_compute_dtype(), str(memory.device),
               self.lm is not None, bool(self.use_hipgraph), fp, self.joint_ctc, float(self.ctc_weight) if self.joint_ctc else None,
               self.ctc_beam)
        if self.ngram_lm is not None:                        # a changed n-gram LM never replays a stale graph (the state pins its table)
            key += (self.ngram_lm.device_table(memory.device).data_ptr(), self.ngram_lm.capacity, self.alpha, self.beta, self.ngram_beam)
        if self.bias is not None:                            # nor does a changed phrase set
            key += (self.bias.device_table(memory.device).data_ptr(), self.bias.capacity, self.bias.n_nodes, self.bias_beam)
        st = self._cached_states.get(key)
        if st is None:
            if len(self._cached_states) >= 4:                # a few shapes; each holds caches + two graphs
                self._cached_states.pop(next(iter(self._cached_states)))
            st = self._cached_states[key] = CachedBeamState(self, b, t, memory.device)
        st.load_memory(memory, memory_mask)
        if head is not None:
            st.joint.load(*head)
        cur, steps = st.run()
        return st.scores[cur], st.preds[cur], steps, b

    def _rescore_outputs(self):
        """the row-padded output layers of the decoder and the LM (_PaddedOutput; None where ops.linear serves), rebuilt when the
        weights or the compute type change"""
        dec, lm = self.model.decoder, self.lm
        ws = [dec.output_layer.weight] + ([lm.output_project.weight] if lm is not None else [])
        key = (ops.get_compute_dtype(),) + tuple((w._version, w.data_ptr()) for w in ws)
        if self._rescore_out is None or self._rescore_out[0] != key:
            self._rescore_out = (key, _padded_output(dec.output_layer.weight, dec.output_layer.bias),
                                 _padded_output(lm.output_project.weight, lm.output_project.bias) if lm is not None else None)
        return self._rescore_out[1:]

    @torch.no_grad()
    def rescore_pass(self, memory, memory_mask, log_probs, lengths, nbest=None):
        """Everything of the two-pass decode behind the CTC head, on the device: the search over log_probs f32 [B, T', V], the pack, the
        decoder (and the LM) over all B x beam_width hypotheses at once, the scoring and the sorted n-best (ops.attention_rescore's
        dict plus 'beam' = the search's own (tokens, out_len, scores)).  No host synchronisation: capturable into one graph once the weight packs exist (after one eager call)."""
        dec, lm, W = self.model.decoder, self.lm, self.beam_width
        V = dec.output_layer.weight.shape[0]
        kw = dict(beam_width=W, cutoff_top_n=self.cutoff_top_n, blank=self.model.assistor.blank)
        ng, ctc, ng_score = self.ngram_lm, None, None
        if self.bias_first_pass:
            # the phrases (and the n-gram) shape the n-best; the second pass takes the acoustic part and scores the strings afresh
            out = ops.ctc_prefix_beam_search_bias(log_probs, lengths, self.bias, ng, self.alpha, self.beta, **kw)
            tokens, out_len, scores = out[:3]
            ctc = scores - out[-1] if ng is None else scores - out[3] - out[4]
            if ng is not None:
                ng_score = ops.ngram_score_sequences(ng, tokens, out_len, self.alpha, self.beta, eos=EOS)
        elif ng is None:
            tokens, out_len, scores = ops.ctc_prefix_beam_search(log_probs, lengths, **kw)
            ctc = scores
        else:
            # the n-gram shapes the n-best; the second pass takes the search's acoustic part and scores the strings afresh (with </s>)
            tokens, out_len, scores, lm_scores = ops.ctc_prefix_beam_search_lm(log_probs, lengths, ng, self.alpha, self.beta, **kw)
            ctc = scores - lm_scores
            ng_score = ops.ngram_score_sequences(ng, tokens, out_len, self.alpha, self.beta, eos=EOS)
        add_score, bias_score = ng_score, None
        if self.bias is not None:                         # the phrases re-rank the n-best, whether or not the first pass saw them
            bias_score = ops.bias_score_sequences(self.bias, tokens, out_len, eos=EOS)
            add_score = bias_score if ng_score is None else ng_score + bias_score
        packed = ops.rescore_pack(tokens, out_len, scores, self.max_len, V, BOS, EOS)
        ys_in = packed[0]
        out_dec, out_lm = self._rescore_outputs()
        logits = _output(out_dec, dec.output_layer, dec.hidden(ys_in, memory, memory_mask, share=W))
        lm_logits = _lm_logits(lm, ys_in, out=out_lm, every=True)
        res = ops.attention_rescore(logits, tokens, out_len, ctc, self.max_len, V, self.ctc_weight, lm_logits=lm_logits,
                                    lm_weight=float(self.lm_weight or 0.0) if lm is not None else 0.0,
                                    nbest=self.nbest if nbest is None else nbest,
                                    penalty=self.penalty, lamda=self.lamda, packed=packed, bos=BOS, eos=EOS, add_score=add_score)
        res['beam'] = (tokens, out_len, scores)           # the first pass, in CTC order
        res['ctc'], res['ng'] = ctc, ng_score             # the terms of total beside att / lm (ng: None without an n-gram LM)
        res['bias'] = bias_score                          # ... and the phrase score (None without a PhraseBias)
        return res

    def _rescore(self, inputs, inputs_mask, nbest=None):
        """the two-pass decode of a batch: encoder, CTC head, rescore_pass (nbest: how many it keeps, None: self.nbest)"""
        memory, memory_mask, _, _ = self.encode(inputs, inputs_mask)
        log_probs, length = self.model.assistor.inference(memory, memory_mask)
        return self.rescore_pass(memory, memory_mask, log_probs.float().contiguous(), length, nbest=nbest)

    @torch.no_grad()
    def recognize_rescore(self, inputs, inputs_mask):
        res = self._rescore(inputs, inputs_mask)
        tok = res['tokens'].cpu()
        preds = torch.cat((tok.masked_fill(tok < 0, EOS), torch.full_like(tok[:, :, :1], EOS)), dim=-1)      # EOS behind every hypothesis
        return self.nbest_translate(preds), res['scores'].cpu()

    @torch.no_grad()
    def recognize(self, inputs, inputs_mask):
        if self.mbr:                                        # the risk-ordered n-best, selected on the device
            tokens, _, scores = self.recognize_tokens(inputs, inputs_mask)
            tok = tokens.cpu()
            return self.nbest_translate(torch.cat((tok, torch.full_like(tok[:, :, :1], EOS)), dim=-1)), scores.cpu()
        if self.rescore:
            return self.recognize_rescore(inputs, inputs_mask)
        if self.apply_cache:
            return self.recognize_cached(inputs, inputs_mask)
        return self._nbest(*self._search(inputs, inputs_mask))

    @torch.no_grad()
    def _search(self, inputs, inputs_mask):
        """the re-forward beam search: (scores [B*beam], prefixes [B*beam, max_len + 2] with BOS, steps, B) on the device"""
        beam = self.beam_width
        memory, memory_mask, _, _ = self.encode(inputs, inputs_mask)
        b, t, v = memory.size()
        R = b * beam
        head = self._ctc_head(memory, memory_mask) if self.joint_ctc else None
        # tile the encoder memory over the beam, like the reference (speech2text.py:51-52)
        beam_memory = memory.unsqueeze(1).repeat([1, beam, 1, 1]).view(R, t, v)
        beam_mask = memory_mask.unsqueeze(1).repeat([1, beam, 1]).view(R, t)
        bs = _BeamState(self, b, t, memory.device, cached=False)
        bs.reset()
        if head is not None:
            bs.joint.load(*head)
        cur, steps = 0, 0
        for step in range(1, self.max_len + 1):
            prefix = bs.preds[cur][:, :step].contiguous()
            logits, _ = self.model.decoder(prefix, beam_memory, beam_mask)       # [R, step, V] fp32
            bs.advance(logits[:, step - 1], _lm_logits(self.lm, prefix), cur, t=step)
            cur ^= 1
            steps = step
            if self.trace is not None:
                self.trace.append((bs.preds[cur][:, :step + 1].clone(), bs.scores[cur].clone()))
            if int(bs.n_fin.item()) == R:           # the reference syncs here every step too (speech2text.py:67)
                break
        return bs.scores[cur], bs.preds[cur], steps, b


class CachedBeamState(_BeamState):
    """Static device state of the cached beam search for one (batch, T', beam, max_len) shape: the beams (_BeamState) and what the
    cache adds to them -- the device position and ancestor tables per phase, write-once self-attention caches for the decoder and the
    LM, per-utterance cross-attention K/V, and the two captured step graphs (even / odd ping-pong phase)."""

    def __init__(self, rec, b, Tm, dev):
        super().__init__(weakref.proxy(rec), b, Tm, dev, cached=True)     # no rec <-> state cycle: graphs die with rec
        dec, lm, R = rec.model.decoder, rec.lm, self.R
        self.maxlen = rec.max_len + 1
        adt = ops.act_dtype()
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)    # noqa: E731
        self.pos = [new((1,), torch.int32) for _ in range(2)]
        self.anc = [new((R, self.maxlen), torch.int32) for _ in range(2)]
        d = dec.d_model
        self.mem_kv = [new((b, Tm, 2 * d), adt) for _ in dec.blocks]
        self.mem_mask = new((b, Tm), torch.uint8)
        self.dec_cache = [(new((R, self.maxlen, d), adt), new((R, self.maxlen, d), adt)) for _ in dec.blocks]
        self.lm_cache = None
        self.lm_recurrent = bool(_lm_recurrent(lm))
        if lm is not None and not self.lm_recurrent:
            dl = lm.embedding.weight.shape[1]
            self.lm_cache = [(new((R, self.maxlen, dl), adt), new((R, self.maxlen, dl), adt)) for _ in lm.blocks]
        self.out_dec = _padded_output(dec.output_layer.weight, dec.output_layer.bias)
        self.out_lm = _padded_output(lm.output_project.weight, lm.output_project.bias) if lm is not None else None
        self.graphs = [None, None]
        self.nf_host = torch.zeros(2, dtype=torch.int32).pin_memory()     # pinned landing pad + events of the lagged all-finished test (run)
        self.nf_ev = [torch.cuda.Event(), torch.cuda.Event()]
        self.warm = [False, False]
        # per layer: may the per-operator step finish it on the fused tail?  Weights, compute dtype, beam and ops._DEC_FUSED decide,
        # all fixed for the state's lifetime (the weights' fingerprint and the compute dtype are part of its cache key)
        self.tail_dec = [self._fused_tail_ok(blk, True) and kv.shape[2] == 512 for blk, kv in zip(dec.blocks, self.mem_kv)]
        self.tail_lm = [self._fused_tail_ok(blk, False) for blk in lm.blocks] if self.lm_cache is not None else []
        # the fused stacks start from the embedded rows' 16-bit twin: decode_embed attaches it whenever is_half(), which
        # act_dtype() == half_dtype() implies, and the compute dtype is part of the cache key -- so step() never checks for it
        self.fused_dec = not dec.normalize_before and adt == ops.half_dtype() and self._fused_stack_ok(dec.blocks, self.tail_dec)
        self.fused_lm = (self.lm_cache is not None and not getattr(lm, 'normalize_before', False) and adt == ops.half_dtype()
                         and self._fused_stack_ok(lm.blocks, self.tail_lm))
        # The LM's layers and the decoder's are two independent chains of small launches (24-80 workgroups on 256 CUs) that only
        # meet at the top-k: the LM chain runs on a side stream, forked at the start of the step and joined before the top-k
        # (in the captured graph: two parallel branches).  Its GEMMs get their own split-K workspace.
        # r06: ONE fork anywhere in a hipGraph takes the whole graph off the runtime's fast per-node path (1.6 -> ~3 us per node,
        # profiles/r06_boundary_probe.txt), which cost this 34-node step about as much as the overlap returned.  Where both stacks run on
        # the fused launches, the LM's layers are the SECOND problem of the decoder's own launches instead (otr_dec_self_step_pair,
        # otr_dec_ffn_fwd_pair, otr_dec_ln_pair: _walk on two chains): the same concurrency, one chain, 23 nodes.
        self.paired = bool(_DECODE_PAIR and self.fused_dec and self.fused_lm and not self.lm_recurrent)
        self.side = torch.cuda.Stream(device=dev) if (lm is not None and not self.paired) else None
        self.side_ws = ops.new_workspace(dev) if self.side is not None else None

    def load_memory(self, memory, memory_mask):
        """Project the encoder memory to cross-attention K|V once per utterance and layer
        (module/attention.py:128-134 does it per hypothesis and per step), then reset the beams."""
        adt = ops.act_dtype()
        for blk, kv in zip(self.rec.model.decoder.blocks, self.mem_kv):
            a = blk.src_attn
            m_kv = ops.linear(memory, a.vk_proj.weight, a.vk_proj.bias, out_dtype=adt)
            kv.copy_(torch.cat((m_kv, m_kv), dim=-1) if a.share_vk_proj else m_kv)
        self.mem_mask.copy_(memory_mask.reshape(self.b, self.Tm))
        self.reset()
        self.pos[0].zero_()

    @staticmethod
    def _close(blk, concat_linear, norm, x, a, ctx):
        """output projection (+ the concat_after Linear) and the add+LayerNorm that closes an attention sub-layer: norm_k of
        a post-norm layer, norm_k+1 of a pre-norm one (nn.TransformerEncoderLayer)"""
        if not blk.concat_after and x.dtype == torch.float32:
            # output projection + residual + LayerNorm as ONE row-block launch (csrc/rowblock.hip), as in training
            packs = ops.proj_ln_packs(x, ctx, a.output_proj.weight, norm.weight)
            if packs is not None:
                return ops.proj_add_layernorm(x, ctx, a.output_proj.weight, a.output_proj.bias, norm.weight, norm.bias, 0.0,
                                              norm.eps, packs)
        att = ops.linear(ctx, a.output_proj.weight, a.output_proj.bias)
        if blk.concat_after:
            att = ops.linear(torch.cat((x, att), dim=-1), concat_linear.weight, concat_linear.bias)
        return ops.add_layernorm(x, att, norm.weight, norm.bias, 0.0, norm.eps)

    @staticmethod
    def _ffn(blk, norm, x):
        ff = blk.feed_forward(x)
        if blk.normalize_before:
            return ops.residual_add(x, ff, 1.0, 0.0)
        return ops.add_layernorm(x, ff, norm.weight, norm.bias, 0.0, norm.eps)

    def _stack_step(self, x, blk, cache, cur, concat_linear=None):
        """self-attention sub-layer of one layer for the new position (encoder/transformer.py:41-56,
        decoder/transformer.py:56-68)"""
        a = blk.slf_attn
        if blk.normalize_before:
            x = ops.add_layernorm(x, None, blk.norm1.weight, blk.norm1.bias, 0.0, blk.norm1.eps)
        qkv = ops.linear(x, a.qvk_proj.weight, a.qvk_proj.bias, out_dtype=ops.act_dtype())
        if a.share_qvk_proj:
            qkv = torch.cat((qkv, qkv, qkv), dim=-1)
        ctx = ops.decode_self_attention(qkv, cache[0], cache[1], self.anc[cur], self.pos[cur], a.nheads)
        return self._close(blk, concat_linear, blk.norm2 if blk.normalize_before else blk.norm1, x, a, ctx)

    def _fused_tail_ok(self, blk, with_cross):
        """can the cross-attention + FFN sub-layers (decoder) / the FFN sub-layer (LM) of this post-norm layer run on the fused decoder
        launches of training (csrc/declayer.hip)?  16-bit mode, d_model 256, 4 heads, GLU, no concat_after, beam <= 32"""
        ff = blk.feed_forward
        if (not ops._DEC_FUSED or not ops.is_half() or blk.normalize_before or blk.concat_after or ff.activation != 'glu'
                or ff.w_1.bias is None or ff.w_2.bias is None or ff.w_1.weight.shape[1] != 256
                or tuple(ff.w_2.weight.shape) != (256, ff.w_1.weight.shape[0] // 2) or self.rec.beam_width > 32):
            return False
        if ops.dec_ffn_slices(ff.w_2.weight.shape[1]) == 0 or ops.ffn_packs(ff.w_1.weight, ff.w_2.weight) is None:
            return False
        if with_cross:
            ca = blk.src_attn
            if ca.nheads != 4 or tuple(ca.q_proj.weight.shape) != (256, 256) or ca.q_proj.bias is None or ca.output_proj.bias is None:
                return False
            if ops.lin_packs(ca.q_proj.weight) is None or ops.lin_packs(ca.output_proj.weight) is None:
                return False
        return True

    def _layer(self, x, blk, cache, cur, tail, concat_self, norm_ffn, kv=None, concat_cross=None):
        """One layer for the new position on the per-operator launches: a decoder layer where kv (its cross-attention K|V) is given,
        an LM layer else.  concat_self / concat_cross: the layer's concat_after Linears, norm_ffn: the norm that closes its FFN.  After
        the self-attention, where `tail` holds, the fused tail: a chain of this one layer that starts at the cross-attention (decoder:
        3 launches for what took 8-9, decoder/transformer.py:70-86) or at the FFN (LM, model/lm.py:94-140: 2 launches)."""
        x = self._stack_step(x, blk, cache, cur, concat_self)
        if tail and ops.lp_of(x) is not None and x.dtype == torch.float32:
            return self._walk([_FusedChain(self, cur, x, [blk], None, None if kv is None else [kv], ops.dec_ffn_slices)], from_self=False)[0]
        if kv is not None:
            a = blk.src_attn
            q = ops.linear(x, a.q_proj.weight, a.q_proj.bias, out_dtype=ops.act_dtype())
            # the beam hypotheses of an utterance are the query rows of ONE attention problem over its memory
            ctx = ops.CrossAttentionFn.apply(q.view(self.b, self.rec.beam_width, -1), kv, self.mem_mask, a.nheads)
            x = self._close(blk, concat_cross, blk.norm3 if blk.normalize_before else blk.norm2, x, a, ctx.view(self.R, -1))
        return self._ffn(blk, norm_ffn, x)

    def _fused_stack_ok(self, blocks, tails):
        """can every layer of this stack run the step on the fused launches (otr_dec_self_step + the fused tail)?"""
        if not _DECODE_STEP_FUSED or not all(tails):
            return False
        for blk in blocks:
            a = blk.slf_attn
            if (a.nheads != 4 or a.share_qvk_proj or tuple(a.qvk_proj.weight.shape) != (768, 256)
                    or tuple(a.output_proj.weight.shape) != (256, 256) or a.qvk_proj.bias is None or a.output_proj.bias is None
                    or ops.lin_packs(a.qvk_proj.weight) is None or ops.lin_packs(a.output_proj.weight) is None):
                return False
        return True

    def _stack_slices(self, F):
        # a few row blocks only: cut the hidden units 16 ways (a workgroup streams its slice of w_1 / w_2 at what ONE CU ingests,
        # 24 workgroups of 393 KB at S = 8); otr_dec_self_step and otr_dec_ln take up to 16 slabs
        return 16 if (F % 2048 == 0 and self.R <= 128) else ops.dec_ffn_slices(F)

    def _dec_chain(self, x, cur):
        return _FusedChain(self, cur, x, self.rec.model.decoder.blocks, self.dec_cache, self.mem_kv, self._stack_slices)

    def _lm_chain(self, x, cur):
        return _FusedChain(self, cur, x, self.rec.lm.blocks, self.lm_cache, None, self._stack_slices)

    def _walk(self, chains, from_self=True):
        """Walk one or two post-norm stacks (_FusedChain) to their ends on the fused launches of csrc/declayer.hip: 3 launches per
        decoder layer, 2 per LM layer (it was 6 and 5: decoder/transformer.py:56-86, encoder/transformer.py:41-63), then the closing
        LayerNorm.  Two chains run in LOCKSTEP: layer i of both in one otr_dec_self_step_pair and one otr_dec_ffn_fwd_pair (the
        decoder's cross-attention launch between them is its own), the closing LayerNorms in one otr_dec_ln_pair; where one stack is
        deeper its tail runs on the single launches.  The same launches on the same operands as one chain at a time: bit-identical
        results.  from_self=False: the first layer starts after its self-attention (the fused tail).  Returns each chain's output."""
        lib, st = L.load(), ops._stream()
        for _ in range(max(len(c.blocks) for c in chains)):
            live = [c for c in chains if c.li < len(c.blocks)]
            if from_self:
                _issue(lib, 'otr_dec_self_step', [c.self_item() for c in live], st)
            for c in live:
                if from_self:
                    c.close(*c.closing)
                c.cross(lib, st)
            _issue(lib, 'otr_dec_ffn_fwd', [c.ffn_item() for c in live], st)
            for c in live:
                c.close(*c.closing)
                c.li += 1
            from_self = True
        if len(chains) == 2:
            L.check(lib.otr_dec_ln_pair(C.byref(chains[0].ln), self.R, C.byref(chains[1].ln), self.R, st), 'otr_dec_ln_pair')
        else:
            L.check(lib.otr_dec_ln(C.byref(chains[0].ln), self.R, st), 'otr_dec_ln')
        return [c.out() for c in chains]

    def _lm_hidden(self, cur):
        """the Transformer LM's rows of the new position for every hypothesis, before its output layer (speech2text.py:108-113)"""
        lm = self.rec.lm
        y = ops.decode_embed(self.preds[cur], self.pos[cur], lm.embedding.weight)
        if self.fused_lm:
            return self._walk([self._lm_chain(y, cur)])[0]
        for blk, cache, tail in zip(lm.blocks, self.lm_cache, self.tail_lm):
            y = self._layer(y, blk, cache, cur, tail, getattr(blk, 'concat_linear', None), blk.norm2)
        return y

    def step(self, cur):
        """One beam-search step (recognize/speech2text.py:95-146) reading phase `cur`, writing phase cur^1.  Three routes: paired (the
        LM's layers ride in the decoder's fused launches), forked (the LM on the side stream), no LM."""
        dec, lm = self.rec.model.decoder, self.rec.lm
        main = torch.cuda.current_stream() if self.side is not None else None      # the forked route's own stream; advance asks for its own
        embed = lambda m: ops.decode_embed(self.preds[cur], self.pos[cur], m.embedding.weight)    # noqa: E731
        lm_logits = None
        if self.paired:
            x, yl = self._walk([self._dec_chain(embed(dec), cur), self._lm_chain(embed(lm), cur)])
            lm_logits = _output(self.out_lm, lm.output_project, yl)
        else:
            if self.side is not None:
                self.side.wait_stream(main)                   # fork
                with torch.cuda.stream(self.side), ops.workspace_lane(self.side_ws):
                    lm_logits = _lm_logits(lm, self.preds[cur], self.pos[cur], self.out_lm, hidden=lambda: self._lm_hidden(cur))
            x = embed(dec)                                    # after the fork: queued before it, the LM branch would wait for it
            if self.fused_dec:
                x = self._walk([self._dec_chain(x, cur)])[0]
            else:
                for blk, cache, kv, tail in zip(dec.blocks, self.dec_cache, self.mem_kv, self.tail_dec):
                    x = self._layer(x, blk, cache, cur, tail, getattr(blk, 'concat_linear1', None), blk.norm3, kv,
                                    getattr(blk, 'concat_linear2', None))
        if dec.normalize_before:
            x = ops.add_layernorm(x, None, dec.after_norm.weight, dec.after_norm.bias, 0.0, dec.after_norm.eps)
        logits = _output(self.out_dec, dec.output_layer, x)       # [R, V], or V padded to a multiple of 8 (_PaddedOutput)
        if self.side is not None:
            main.wait_stream(self.side)                   # join: the LM's logits are ready
        self.advance(logits, lm_logits, cur, pos=self.pos, anc=self.anc, maxlen=self.maxlen)

    def _launch(self, cur):
        if not self.rec.use_hipgraph:
            return self.step(cur)
        if self.graphs[cur] is not None:
            return self.graphs[cur].replay()
        if not self.warm[cur]:            # first visit runs eagerly: creates weight shadows, workspace, allocator state
            self.warm[cur] = True
            return self.step(cur)
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            self.step(cur)
        self.graphs[cur] = g
        g.replay()

    def run(self):
        cur, steps = 0, 0
        if self.rec.trace is not None or not _DECODE_LAGGED_STOP:
            for step in range(1, self.rec.max_len + 1):
                self._launch(cur)
                cur ^= 1
                steps = step
                if self.rec.trace is not None:
                    self.rec.trace.append((self.preds[cur][:, :step + 1].clone(), self.scores[cur].clone()))
                if int(self.n_fin[cur, 0].item()) == self.R:  # the reference syncs here every step too (speech2text.py:67)
                    break
            return cur, steps
        # r06: the all-finished count of step s is read AFTER step s + 1 has been queued.  The per-step sync was a host round trip between
        # two replayed steps (rocprofv3: the 4 us device-to-host copy, then 18 us of nothing until the next graph's first kernel: 6 % of a
        # 0.29 ms step).  At most one step runs in vain; it reads phase A and writes phase B, so the finished state in A is what is returned
        # -- the same hypotheses and scores as the synchronous loop (tests/test_gpu_decode.py, test_gpu_round6.py).
        # The count goes home as a 4-byte copy queued behind the step on the SAME stream (4 us + a ~6 us gap per step by rocprofv3).  Measured
        # and not kept: the copy on a side stream behind an event (0.32 ms per step against 0.28: a cross-stream wait per step costs more than
        # the copy, like every fork of DESIGN.md 5.8); the copy as a node of the step's own graph (the same 0.28); the prune launch's last
        # workgroup storing the count straight to pinned host memory, no copy at all (the same 0.28 within the run-to-run noise).
        nf, ev = self.nf_host, self.nf_ev
        for step in range(1, self.rec.max_len + 1):
            self._launch(cur)
            cur ^= 1
            steps = step
            nf[cur:cur + 1].copy_(self.n_fin[cur, :1], non_blocking=True)
            ev[cur].record()
            if step > 1:
                ev[cur ^ 1].synchronize()
                if int(nf[cur ^ 1]) == self.R:
                    return cur ^ 1, step - 1
        return cur, steps


class CTCRecognizer(Recognizer):
    """recognize/ctc.py:7-67.  `model` must expose frontend / encoder / assistor.
    mode 'greedy': per-frame arg-max, repeats and blanks collapsed.  mode 'beam': CTC prefix beam search on the device
    (ops.ctc_prefix_beam_search; cutoff_top_n defaults to 40 as in ctcdecode.CTCBeamDecoder) in place of the reference's ctcdecode_edited; the
    1-best of the beam.  The two differ in general, also at beam_width 1: the beam sums the probability of every path of a prefix,
    greedy follows the single best path.  ngram_lm: None, or an ngram.NGramLM (a backoff n-gram over the units, NGramLM.from_arpa):
    in beam mode every extension then gains alpha * ln P_LM + beta inside the search (ops.ctc_prefix_beam_search_lm), ctcdecode's
    character-based scorer; greedy mode ignores it, as the reference does.  A path is not loaded here (build_recognizer does that);
    without an LM alpha / beta are unused, as in ctcdecode without a scorer.  lm / lm_weight are unused in beam mode as in the
    reference.  bias: None, or a bias.PhraseBias over the CTC head's units (phrase biasing, "hotwords"): in beam mode every extension
    s -> s c then gains psi_minus(state(s c)) - psi(state(s)) inside the search, behind the n-gram's addend if any, and a match left
    open at the end of the utterance is refunded (ops.ctc_prefix_beam_search_bias; include/otrans_hip.h otr_ctc_beam_search_bias).
    Greedy mode ignores bias, as it ignores ngram_lm.  The alignment of recognize_with_times runs on the acoustic log-probs alone.
    mbr=True (beam mode only): the beam_width hypotheses of the search are re-ordered by ascending risk under softmax(mbr_scale *
    score), as SpeechToTextRecognizer does, and the 1-best everywhere is the hypothesis of least risk.  recognize_with_confidence gives
    the 1-best's tokens the posterior mass that agrees with them (beam mode only: greedy decoding has no beam to take a consensus of)."""

    def __init__(self, model, lm=None, lm_weight=0.1, ngram_lm=None, beam_width=5, idx2unit=None, ngpu=1,
                 mode='greedy', alpha=0.1, beta=0.0, cutoff_top_n=40, bias=None, mbr=False, mbr_scale=1.0):
        super().__init__(model, idx2unit, lm, lm_weight, ngpu)
        if mbr and mode != 'beam':
            raise ValueError("CTCRecognizer: mbr=True needs mode='beam': greedy decoding has no beam to take a consensus of")
        self.mbr, self.mbr_scale = _mbr_args('CTCRecognizer', mbr, mbr_scale, beam_width)
        if mode not in ('greedy', 'beam'):
            raise NotImplementedError("CTCRecognizer mode '%s': 'greedy' and 'beam' are built" % mode)
        if mode == 'beam' and ngram_lm is not None and not isinstance(ngram_lm, NGramLM):
            raise NotImplementedError('CTCRecognizer: ngram_lm must be an NGramLM, not %s: load the ARPA file with '
                                      'NGramLM.from_arpa(path, idx2unit) (KenLM binaries are not read)' % type(ngram_lm).__name__)
        if bias is not None and not isinstance(bias, PhraseBias):
            raise TypeError('CTCRecognizer: bias must be a PhraseBias, not %s: build one with PhraseBias(phrases, vocab_size) or '
                            'PhraseBias.from_texts(lines, idx2unit)' % type(bias).__name__)
        self.bias = bias
        self.beam_width, self.mode, self.ngram_lm = beam_width, mode, ngram_lm
        self.alpha, self.beta, self.cutoff_top_n = alpha, beta, cutoff_top_n

    def _encode(self, inputs, inputs_mask):
        x, mask, _ = self.model.frontend.inference(inputs, inputs_mask, None)
        memory, memory_mask, _ = self.model.encoder(x, mask)
        return memory, memory_mask

    def _greedy(self, memory, memory_mask):
        """the greedy decode of the CTC head's logits (no look-ahead; argmax(log_softmax) == argmax): the per-frame arg-max on the
        device, repeats and PAD collapsed on the host.  Returns (lists, logits [B, T', V], frames [B])"""
        logits = self.model.assistor.compute_logits(memory)
        B, T, V = logits.shape
        best_s = torch.empty((B * T, 1), dtype=torch.float32, device=logits.device)
        best_i = torch.empty((B * T, 1), dtype=torch.long, device=logits.device)
        L.check(L.load().otr_beam_topk(_ptr(logits), V, None, 0, 0.0, B * T, V, 1, _ptr(best_s), _ptr(best_i),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'otr_beam_topk')
        length = memory_mask.sum(-1)
        best, n = best_i.view(B, T).cpu(), length.cpu()
        lists = []
        for b in range(B):
            pred, last_k = [], PAD
            for k in best[b, :int(n[b])].tolist():
                if k != last_k and k != PAD:
                    pred.append(k)
                last_k = k
            lists.append(pred)
        return lists, logits, length

    @staticmethod
    def _best_lists(tokens, out_len):
        """the 1-best of the beam as host lists"""
        best, n = tokens[:, 0].cpu(), out_len[:, 0].cpu()
        return [best[b, :int(n[b])].tolist() for b in range(best.size(0))]

    @staticmethod
    def _padded(lists, dev):
        """host lists -> (tokens int64 [B, width >= 1] padded with PAD, lengths int32 [B]) on `dev`"""
        width = max([len(p) for p in lists] + [1])
        tokens = torch.tensor([p + [PAD] * (width - len(p)) for p in lists], dtype=torch.long)
        return tokens.to(dev), torch.tensor([len(p) for p in lists], dtype=torch.int32).to(dev)

    @torch.no_grad()
    def recognize_greedy(self, inputs, inputs_mask):
        return self._greedy(*self._encode(inputs, inputs_mask))[0]

    @torch.no_grad()
    def recognize_beam(self, inputs, inputs_mask):
        memory, memory_mask = self._encode(inputs, inputs_mask)
        log_probs, length = self.model.assistor.inference(memory, memory_mask)      # look-ahead conv + log_softmax, f32
        return self._best_lists(*self._beam(log_probs, length))

    def _beam(self, log_probs, length, with_scores=False):
        """the beam of the CTC head's log-probs, with the n-gram LM and the phrases fused in where they were given: (tokens, out_len[,
        scores]), in ascending order of risk with mbr=True"""
        out = self._beam_search(log_probs, length)
        if self.mbr:
            out = _consensus_nbest(out[0], out[1].to(torch.int32), out[2].float(), self.mbr_scale, True, self.beam_width, -1)
        return out[:3 if with_scores else 2]

    def _beam_search(self, log_probs, length):
        """the search's own (tokens, out_len, scores), best score first"""
        kw = dict(beam_width=self.beam_width, cutoff_top_n=self.cutoff_top_n, blank=self.model.assistor.blank)
        if self.bias is not None:
            return ops.ctc_prefix_beam_search_bias(log_probs, length, self.bias, self.ngram_lm, self.alpha, self.beta, **kw)[:3]
        if self.ngram_lm is None:
            return ops.ctc_prefix_beam_search(log_probs, length, **kw)[:3]
        return ops.ctc_prefix_beam_search_lm(log_probs, length, self.ngram_lm, self.alpha, self.beta, **kw)[:3]

    @torch.no_grad()
    def recognize_tokens_with_confidence(self, inputs, inputs_mask):
        """recognize_tokens() plus the consensus of the search's beam_width hypotheses (ops.nbest_consensus at mbr_scale), on the device:
        (tokens [B, 1, L], lengths [B, 1], scores [B, 1] of the 1-best -- the hypothesis of least risk with mbr=True --, conf f32 [B, L]:
        per token the posterior mass of the hypotheses whose alignment matches it, post f32 [B]: the 1-best's own posterior)."""
        if self.mode != 'beam':
            raise ValueError("CTCRecognizer: confidences need mode='beam': greedy decoding has no beam to take a consensus of")
        memory, memory_mask = self._encode(inputs, inputs_mask)
        log_probs, length = self.model.assistor.inference(memory, memory_mask)
        tokens, out_len, scores = self._beam_search(log_probs, length)
        return _consensus_nbest(tokens, out_len.to(torch.int32), scores.float(), self.mbr_scale, self.mbr, 1, -1)

    @torch.no_grad()
    def recognize_with_confidence(self, inputs, inputs_mask):
        """recognize() with token confidences: (texts, confidences: per utterance [(unit, confidence), ...] for the 1-best, its units
        read in order being the words of its text as in recognize_with_times, utt_posterior: the 1-best's posterior, a host tensor [B])"""
        tokens, lengths, _, conf, post = self.recognize_tokens_with_confidence(inputs, inputs_mask)
        tok, n, conf = tokens[:, 0].cpu(), lengths[:, 0].cpu(), conf.cpu()
        preds = [tok[b, :int(n[b])].tolist() for b in range(tok.size(0))]
        confidences = []
        for b, pred in enumerate(preds):
            items = []
            for k, t in enumerate(pred):                   # translate()'s walk: a list ends before its first EOS and skips PAD
                if t == EOS:
                    break
                if t != PAD:
                    items.append((self.idx2unit[t], float(conf[b, k])))
            confidences.append(items)
        return self.translate(preds), confidences, post.cpu()

    @torch.no_grad()
    def recognize_tokens(self, inputs, inputs_mask):
        """recognize() as device tensors (tokens int64 [B, 1, L], lengths int32 [B, 1], scores f32 [B, 1]) for ops.edit_distance /
        evaluate.ErrorRateMeter; translate(tokens[b, 0, :lengths[b, 0]]) gives recognize()'s strings.  Beam mode: the search's own
        outputs narrowed to the 1-best, nothing goes through the host.  Greedy mode: the collapse of repeats and blanks is the host
        loop of _greedy, its lists padded with PAD and uploaded (one host round trip per batch); the score is 0."""
        memory, memory_mask = self._encode(inputs, inputs_mask)
        if self.mode == 'beam':
            log_probs, length = self.model.assistor.inference(memory, memory_mask)
            tokens, out_len, scores = self._beam(log_probs, length, with_scores=True)
            return tokens[:, :1], out_len[:, :1].to(torch.int32), scores[:, :1].float()
        tokens, lengths = self._padded(self._greedy(memory, memory_mask)[0], inputs.device)
        return tokens.unsqueeze(1), lengths.unsqueeze(1), torch.zeros((tokens.size(0), 1), dtype=torch.float32, device=inputs.device)

    def recognize(self, inputs, inputs_mask):
        if self.mode == 'beam':
            return self.translate(self.recognize_beam(inputs, inputs_mask))
        return self.translate(self.recognize_greedy(inputs, inputs_mask))

    def _span_lists(self, labels, labels_length, spans, label_logp, score):
        """per utterance [(unit, start_frame, end_frame, logp), ...]; like translate() a list ends before its first EOS and skips PAD;
        an utterance that could not be aligned (score -inf) gives an empty list"""
        labels, n, spans, label_logp, score = labels.cpu(), labels_length.cpu(), spans.cpu(), label_logp.cpu(), score.cpu()
        out = []
        for b in range(labels.size(0)):
            items = []
            for j in range(int(n[b]) if score[b] > -float('inf') else 0):
                k = int(labels[b, j])
                if k == EOS:
                    break
                if k == PAD:
                    continue
                items.append((self.idx2unit[k], int(spans[b, j, 0]), int(spans[b, j, 1]), float(label_logp[b, j])))
            out.append(items)
        return out

    @torch.no_grad()
    def align(self, inputs, inputs_mask, labels, labels_length):
        """CTC forced alignment of known transcripts: `labels` [B, max_tgt] unit ids without BOS / EOS, `labels_length` [B] their counts
        (at most 127).  Per utterance a list of (unit, start_frame, end_frame, logp): the encoder frames [start, end) the most probable
        CTC path gives the unit, and the unit's log-probs summed over them; frames_to_seconds() turns a frame into a time."""
        memory, memory_mask = self._encode(inputs, inputs_mask)
        _, spans, label_logp, score = self.model.assistor.align(memory, memory_mask, labels, labels_length)
        return self._span_lists(labels, labels_length, spans, label_logp, score)

    @torch.no_grad()
    def recognize_with_times(self, inputs, inputs_mask):
        """recognize() with time stamps (what ctcdecode's `timesteps` give the reference's users): one encoder pass, greedy or beam
        decoding as `mode` says, then the 1-best aligned on the log-probs it was decoded from.  Returns (texts, per-utterance lists of
        (unit, start_frame, end_frame, logp)); the units of a list, read in order, are the words of its text."""
        memory, memory_mask = self._encode(inputs, inputs_mask)
        if self.mode == 'beam':
            log_probs, length = self.model.assistor.inference(memory, memory_mask)
            preds = self._best_lists(*self._beam(log_probs, length))       # the alignment below runs on the acoustic log-probs alone
        else:
            preds, logits, length = self._greedy(memory, memory_mask)
            log_probs = ops.log_softmax(logits)
        labels, labels_length = self._padded(preds, log_probs.device)
        if labels.size(1) > ops.CTC_ALIGN_MAX_TGT:
            raise ValueError('recognize_with_times: a 1-best of %d units, the alignment takes at most %d'
                             % (labels.size(1), ops.CTC_ALIGN_MAX_TGT))
        _, spans, label_logp, score = ops.ctc_forced_align(log_probs, length, labels, labels_length, blank=self.model.assistor.blank)
        return self.translate(preds), self._span_lists(labels, labels_length, spans, label_logp, score)


def frames_to_seconds(frame, subsample=4, frame_shift_ms=10.0):
    """Start time, in seconds, of the input window of encoder frame `frame` (a span's end_frame gives the start of the first frame
    after the unit).  The ConvFrontEnd built here is two stride-2 convolutions, so an encoder frame advances subsample = 4 feature
    frames of frame_shift_ms each; a frontend with another stride passes its own product."""
    return frame * subsample * frame_shift_ms / 1000.0


def build_recognizer(model_type, model, lm, args, idx2unit):
    """recognize/__init__.py:5-16."""
    if model_type == 'speech2text':
        ngram_lm = getattr(args, 'ngram_lm', None)
        if isinstance(ngram_lm, str):
            ngram_lm = NGramLM.from_arpa(ngram_lm, idx2unit)
        kw = {k: getattr(args, k) for k in ('alpha', 'beta') if hasattr(args, k)}
        bias = getattr(args, 'bias_phrases', None)
        if isinstance(bias, str):                                               # a text file: one phrase per line
            with open(bias, encoding='utf-8') as f:
                bias = PhraseBias.from_texts(f, idx2unit, score=getattr(args, 'bias_score', 2.0),
                                             vocab_size=model.decoder.output_layer.weight.shape[0])
        return SpeechToTextRecognizer(model=model, lm=lm, lm_weight=args.lm_weight, ctc_weight=args.ctc_weight,
                                      beam_width=args.beam_width, nbest=args.nbest, max_len=args.max_len,
                                      idx2unit=idx2unit, penalty=args.penalty, lamda=args.lamda, ngpu=args.ngpu,
                                      joint_ctc=getattr(args, 'joint_ctc', False), ctc_beam=getattr(args, 'ctc_beam', None),
                                      rescore=getattr(args, 'rescore', False), ngram_lm=ngram_lm,
                                      ngram_beam=getattr(args, 'ngram_beam', None), bias=bias,
                                      bias_beam=getattr(args, 'bias_beam', None),
                                      bias_first_pass=getattr(args, 'bias_first_pass', False), mbr=getattr(args, 'mbr', False),
                                      mbr_scale=getattr(args, 'mbr_scale', 1.0), **kw)
    if model_type == 'ctc':
        ngram_lm = args.ngram_lm
        if isinstance(ngram_lm, str):                                           # the reference passes the path on to ctcdecode
            ngram_lm = NGramLM.from_arpa(ngram_lm, idx2unit)
        bias = getattr(args, 'bias_phrases', None)
        if isinstance(bias, str):                                               # a text file: one phrase per line
            with open(bias, encoding='utf-8') as f:
                bias = PhraseBias.from_texts(f, idx2unit, score=getattr(args, 'bias_score', 2.0),
                                             vocab_size=model.assistor.output_layer.weight.shape[0])
        return CTCRecognizer(model=model, lm=lm, lm_weight=args.lm_weight, ngram_lm=ngram_lm,
                             beam_width=args.beam_width, idx2unit=idx2unit, ngpu=args.ngpu, mode=args.mode,
                             alpha=args.alpha, beta=args.beta, bias=bias, mbr=getattr(args, 'mbr', False),
                             mbr_scale=getattr(args, 'mbr_scale', 1.0))
    if model_type == 'transducer':
        from .transducer import TransducerRecognizer          # transducer.py imports this module
        return TransducerRecognizer(model=model, idx2unit=idx2unit, max_symbols=getattr(args, 'max_symbols', 4),
                                    max_len=getattr(args, 'max_len', 200), ngpu=getattr(args, 'ngpu', 1),
                                    mode=getattr(args, 'mode', 'greedy'), beam_width=getattr(args, 'beam_width', 4),
                                    nbest=getattr(args, 'nbest', 1), mbr=getattr(args, 'mbr', False),
                                    mbr_scale=getattr(args, 'mbr_scale', 1.0))
    raise NotImplementedError
