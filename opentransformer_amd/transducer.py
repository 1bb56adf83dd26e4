"""The transducer (RNN-T): frontend + encoder, an LSTM predictor over the label history, and a joint network over every (frame,
label position) pair, trained on the lattice likelihood and decoded greedily, frame-synchronously.  The reference project has no
transducer; the definitions are those of include/otrans_hip.h (otr_rnnt_*) and the tests restate them in float64.

  predictor  nn.Embedding(V, E) -> nn.LSTM(E, H, num_layers, batch_first, dropout), a parameter container: training runs it through
             ops.embedding + ops.lstm_layer time-major from the zero state, as RecurrentLanguageModel._train_forward does; decoding
             runs one cell step per launch group (ops.decode_lookup, two ops.linear and ops.lstm_cell per layer)
  joint      z = tanh(enc_proj(memory)[:, :, None] + pred_proj(g)[:, None]) (ops.rnnt_joint), logits = output(z): f32 [B, T', U + 1, V]
  loss       ops.rnnt_loss on the raw logits: blank = BLK = 0, labels truth[:, 1:-1] with targets_length - 1 of them (what CTCModel
             takes), the predictor reads truth[:, :-1] = [BOS, y_1 .. y_U]
"""
import torch
import torch.nn as nn

from . import ops
from .model import AcousticModel, BuildEncoder, BuildFrontEnd, End2EndModel
from .nn import BLK, BOS
from .recognize import Recognizer, _consensus_nbest, _mbr_args


class TransducerPredictor(nn.Module):
    """nn.Embedding + nn.LSTM over [BOS, y_1 .. y_U]; state_dict keys `embedding.weight`, `rnn.weight_ih_l0` ..."""

    def __init__(self, vocab_size, embedding_size, hidden_size, num_layers=1, dropout=0.0):
        super().__init__()
        self.num_layers, self.hidden_size, self.dropout = num_layers, hidden_size, float(dropout)
        self.embedding = nn.Embedding(vocab_size, embedding_size)
        self.rnn = nn.LSTM(input_size=embedding_size, hidden_size=hidden_size, num_layers=num_layers, batch_first=True,
                           dropout=dropout if num_layers > 1 else 0.0, bidirectional=False)

    def layer_params(self, k):
        r = self.rnn
        return (getattr(r, 'weight_ih_l%d' % k), getattr(r, 'weight_hh_l%d' % k), getattr(r, 'bias_ih_l%d' % k), getattr(r, 'bias_hh_l%d' % k))

    def forward(self, tokens):
        """tokens [B, U + 1] -> g TIME-MAJOR [U + 1, B, H] with its 16-bit twin; nothing is packed: the LSTM is causal, so what
        it computes behind a row's length never reaches a position inside it"""
        x = ops.embedding(tokens.t(), self.embedding.weight)
        for k in range(self.num_layers):
            if k:
                x = ops.dropout(x, self.dropout, self.training)
            x = ops.lstm_layer(x, *self.layer_params(k))
        return x

    @torch.no_grad()
    def step(self, tokens, h, c):
        """one step for all rows: tokens int64 [B, 1], h / c lists per layer or None (the zero state) -> (h', c') as new lists"""
        nl = self.num_layers
        h = list(h) if h is not None else [None] * nl
        c = list(c) if c is not None else [None] * nl
        x = ops.decode_lookup(tokens, None, self.embedding.weight)
        for k in range(nl):
            w_ih, w_hh, b_ih, b_hh = self.layer_params(k)
            ga = ops.linear(x, w_ih, b_ih)
            gb = ops.linear(h[k], w_hh, b_hh) if h[k] is not None else None
            h[k], c[k] = ops.lstm_cell(ga, gb, b_hh if gb is None else None, c[k])
            x = h[k]
        return h, c


class TransducerJoint(nn.Module):
    """enc_proj Linear(d -> J), pred_proj Linear(H -> J, no bias), output Linear(J -> V)"""

    def __init__(self, encoder_size, predictor_size, joint_size, vocab_size):
        super().__init__()
        if joint_size < 4 or joint_size % 4:
            raise ValueError('TransducerJoint: joint_size=%d must be a positive multiple of 4' % joint_size)
        self.enc_proj = nn.Linear(encoder_size, joint_size)
        self.pred_proj = nn.Linear(predictor_size, joint_size, bias=False)
        self.output = nn.Linear(joint_size, vocab_size)

    def project_encoder(self, memory):
        return ops.linear(memory, self.enc_proj.weight, self.enc_proj.bias)

    def project_predictor(self, g):
        return ops.linear(g, self.pred_proj.weight)

    def logits(self, z):
        return ops.linear(z, self.output.weight, self.output.bias)

    def forward(self, memory, memory_length, g_tm, labels_length):
        """memory [B, T', d], g_tm time-major [U + 1, B, H] -> raw logits f32 [B, T', U + 1, V]"""
        pe = self.project_encoder(memory)
        pg = self.project_predictor(g_tm).transpose(0, 1)
        return self.logits(ops.rnnt_joint(pe, pg, memory_length, labels_length))


class TransducerModel(AcousticModel):
    """forward(inputs, targets) -> (loss, None): the transducer loss of the batch, 'mean' over the utterances (an utterance the loss
    kernel guards counts with 0, as CTC's zero_infinity does).  The fp16 loss scale rides in the loss launch's gradient."""

    def __init__(self, params):
        super().__init__()
        self.frontend = BuildFrontEnd[params['frontend_type']](**params['frontend'])
        self.encoder = BuildEncoder[params['encoder_type']](**params['encoder'])
        self.vocab_size = params['vocab_size']
        p = params['predictor']
        self.predictor = TransducerPredictor(self.vocab_size, p['embedding_size'], p['hidden_size'], p.get('num_layers', 1),
                                             p.get('dropout', 0.0))
        self.joint = TransducerJoint(params['encoder_output_size'], p['hidden_size'], params['joint_size'], self.vocab_size)

    def teacher_forced_logits(self, memory, memory_mask, targets):
        """(logits [B, T', U + 1, V], memory_length, labels: the view truth[:, 1:-1], labels_length)"""
        truth, truth_length = targets['targets'], targets['targets_length']
        memory_length = torch.sum(memory_mask, dim=-1)
        labels, labels_length = truth[:, 1:-1], truth_length.add(-1)
        g = self.predictor(truth[:, :-1])
        return self.joint(memory, memory_length, g, labels_length), memory_length, labels, labels_length

    def forward(self, inputs, targets):
        memory, memory_mask = self.encode(inputs['inputs'], inputs['mask'])
        logits, memory_length, labels, labels_length = self.teacher_forced_logits(memory, memory_mask, targets)
        loss, _ = ops.rnnt_loss(logits, memory_length, labels, labels_length, blank=BLK, grad_scale=ops.loss_scale_of(self))
        return loss, None

    @torch.no_grad()
    def predictor_step(self, tokens, h, c):
        """ops.rnnt_greedy's predictor_step: (h', c', pg' [B, J])"""
        h, c = self.predictor.step(tokens, h, c)
        return h, c, self.joint.project_predictor(h[-1])

    def save_checkpoint(self, params, name):
        torch.save({'params': params, 'frontend': self.frontend.state_dict(), 'encoder': self.encoder.state_dict(),
                    'predictor': self.predictor.state_dict(), 'joint': self.joint.state_dict()}, name)

    def load_model(self, chkpt):
        self.frontend.load_state_dict(chkpt['frontend'])
        self.encoder.load_state_dict(chkpt['encoder'])
        self.predictor.load_state_dict(chkpt['predictor'])
        self.joint.load_state_dict(chkpt['joint'])


End2EndModel['transducer'] = TransducerModel


class TransducerRecognizer(Recognizer):
    """Greedy frame-synchronous decoding (ops.rnnt_greedy): at every frame the arg-max of the joint is emitted and fed back to the
    predictor until it is blank or `max_symbols` tokens came out of that frame; a hypothesis ends with its frames or at `max_len`
    tokens.  The score is the sum of the log-probs of every decision, blanks included.
    mode 'beam': ops.rnnt_beam at `beam_width` -- frame-synchronous with at most ONE symbol per frame, identical hypotheses merged
    before pruning; the 1-best everywhere, the `nbest` best from recognize_tokens.  Its score is the log of the summed probability
    of the alignments the search kept, not greedy's score: greedy pays a blank to leave a frame after an emission, the beam does
    not.  beam_width=1 is one-symbol-per-frame arg-max decoding, which is not mode 'greedy' at max_symbols=1 either: after an
    emission greedy looks at the same frame again and is forced to its blank, the beam moves on.  max_symbols keeps its meaning
    in greedy mode and is unused in beam mode; beam mode takes max_len up to ops.RNNT_BEAM_MAX_LEN.  beam_width and nbest are unused
    and unchecked in greedy mode (an args namespace shared with the other recognizers builds the greedy recognizer it always built):
    greedy decoding has one hypothesis, and recognize_tokens returns that one.
    mbr=True (beam mode only): the beam_width hypotheses of the search are re-ordered by ascending risk under softmax(mbr_scale *
    score), as the other recognizers do, and the 1-best everywhere is the hypothesis of least risk; the frames follow the same
    permutation.  recognize_with_confidence gives the 1-best's tokens the posterior mass that agrees with them (beam mode only)."""

    def __init__(self, model, idx2unit=None, max_symbols=4, max_len=200, ngpu=1, mode='greedy', beam_width=4, nbest=1, mbr=False,
                 mbr_scale=1.0):
        super().__init__(model, idx2unit, None, None, ngpu)
        if not isinstance(model, TransducerModel):
            raise TypeError('TransducerRecognizer: model must be a TransducerModel, not %s' % type(model).__name__)
        if mbr and mode != 'beam':
            raise ValueError("TransducerRecognizer: mbr=True needs mode='beam': greedy decoding has no beam to take a consensus of")
        if mode not in ('greedy', 'beam'):
            raise NotImplementedError("TransducerRecognizer mode '%s': 'greedy' and 'beam' are built" % mode)
        self.max_symbols, self.max_len = int(max_symbols), int(max_len)
        self.mode, self.beam_width, self.nbest = mode, int(beam_width), int(nbest)
        if mode == 'beam':                                  # greedy mode ignores beam_width and nbest, whatever they are
            if not 1 <= self.beam_width <= ops.RNNT_BEAM_MAX:
                raise ValueError('TransducerRecognizer: beam_width=%d must be in [1, %d]' % (self.beam_width, ops.RNNT_BEAM_MAX))
            if not 1 <= self.nbest <= self.beam_width:
                raise ValueError('TransducerRecognizer: nbest=%d must be in [1, beam_width=%d]' % (self.nbest, self.beam_width))
            ops.rnnt_beam_limits('TransducerRecognizer', self.beam_width, self.max_len)
        self.mbr, self.mbr_scale = _mbr_args('TransducerRecognizer', mbr, mbr_scale, self.beam_width)

    def _project(self, inputs, inputs_mask):
        x, mask, _ = self.model.frontend.inference(inputs, inputs_mask, None)
        memory, memory_mask, _ = self.model.encoder(x, mask)
        memory_length = torch.sum(memory_mask.squeeze(1) if memory_mask.dim() == 3 else memory_mask, dim=-1)
        return self.model.joint.project_encoder(memory), memory_length.to(torch.int32)

    @torch.no_grad()
    def _beam_search(self, inputs, inputs_mask):
        """the search's own beam, best score first: (tokens int64 [B, W, L], lengths int32 [B, W], scores f32 [B, W], frames int32
        [B, W, L]) on the device"""
        pe, memory_length = self._project(inputs, inputs_mask)
        return ops.rnnt_beam(pe, memory_length, self.model.predictor_step, self.model.joint.logits, beam_width=self.beam_width,
                             max_len=self.max_len, blank=BLK, bos=BOS)

    def _beam(self, inputs, inputs_mask, n):
        """the n best of the beam with their frames, and the consensus of the whole beam: (tokens [B, n, L], lengths [B, n], scores
        [B, n], frames [B, n, L], conf [B, L], post [B]); in ascending order of risk with mbr=True, by score otherwise"""
        tokens, lengths, scores, frames = self._beam_search(inputs, inputs_mask)
        tok, ln, sc, conf, post, fr = _consensus_nbest(tokens, lengths, scores, self.mbr_scale, self.mbr, n, -1, follow=frames)
        return tok, ln, sc, fr, conf, post

    @torch.no_grad()
    def _decode(self, inputs, inputs_mask):
        """(tokens int64 [B, L], lengths int32 [B], scores f32 [B], frames int32 [B, L]) of the 1-best, on the device"""
        if self.mode == 'beam':
            if self.mbr:
                tokens, lengths, scores, frames = self._beam(inputs, inputs_mask, 1)[:4]
            else:
                tokens, lengths, scores, frames = self._beam_search(inputs, inputs_mask)
            return tokens[:, 0], lengths[:, 0], scores[:, 0], frames[:, 0]
        pe, memory_length = self._project(inputs, inputs_mask)
        return ops.rnnt_greedy(pe, memory_length, self.model.predictor_step, self.model.joint.logits,
                               max_symbols=self.max_symbols, max_len=self.max_len, blank=BLK, bos=BOS)

    def recognize_tokens(self, inputs, inputs_mask):
        """(tokens int64 [B, N, L], lengths int32 [B, N], scores f32 [B, N]) for ops.edit_distance / evaluate.evaluate: N = 1 in greedy
        mode, nbest in beam mode (in ascending order of risk with mbr=True)"""
        if self.mode == 'beam':
            if self.mbr:
                return self._beam(inputs, inputs_mask, self.nbest)[:3]
            tokens, lengths, scores, _ = self._beam_search(inputs, inputs_mask)
            return tokens[:, :self.nbest], lengths[:, :self.nbest], scores[:, :self.nbest]
        tokens, lengths, scores, _ = self._decode(inputs, inputs_mask)
        return tokens.unsqueeze(1), lengths.unsqueeze(1), scores.unsqueeze(1)

    @torch.no_grad()
    def recognize_tokens_with_confidence(self, inputs, inputs_mask):
        """recognize_tokens() narrowed to the 1-best plus the consensus of the search's beam_width hypotheses (ops.nbest_consensus at
        mbr_scale), on the device: (tokens [B, 1, L], lengths [B, 1], scores [B, 1] of the 1-best -- the hypothesis of least risk with
        mbr=True --, conf f32 [B, L]: per token the posterior mass of the hypotheses whose alignment matches it, post f32 [B]: the
        1-best's own posterior)."""
        if self.mode != 'beam':
            raise ValueError("TransducerRecognizer: confidences need mode='beam': greedy decoding has no beam to take a consensus of")
        tokens, lengths, scores, _, conf, post = self._beam(inputs, inputs_mask, 1)
        return tokens, lengths, scores, conf, post

    @torch.no_grad()
    def recognize_with_confidence(self, inputs, inputs_mask):
        """recognize() with token confidences: (texts, confidences: per utterance [(unit, confidence), ...] for the 1-best, its units
        read in order being the words of its text as in recognize_with_times, utt_posterior: the 1-best's posterior, a host tensor [B])"""
        tokens, lengths, _, conf, post = self.recognize_tokens_with_confidence(inputs, inputs_mask)
        preds, conf = self._lists(tokens[:, 0], lengths[:, 0]), conf.cpu()
        confidences = []
        for b, pred in enumerate(preds):
            items = []
            for k, t in enumerate(pred):                   # translate()'s walk: a list ends before its first EOS and skips PAD
                if t == BOS:
                    break
                if t != BLK:
                    items.append((self.idx2unit[t], float(conf[b, k])))
            confidences.append(items)
        return self.translate(preds), confidences, post.cpu()

    def _lists(self, tokens, lengths):
        tok, n = tokens.cpu(), lengths.cpu()
        return [tok[b, :int(n[b])].tolist() for b in range(tok.size(0))]

    def recognize(self, inputs, inputs_mask):
        tokens, lengths, _, _ = self._decode(inputs, inputs_mask)
        return self.translate(self._lists(tokens, lengths))

    def recognize_with_times(self, inputs, inputs_mask):
        """(texts, per utterance [(unit, frame), ...]): the encoder frame at which each unit was emitted (recognize.frames_to_seconds
        turns it into a time); the units of a list, read in order, are the words of its text"""
        tokens, lengths, _, frames = self._decode(inputs, inputs_mask)
        preds, fr = self._lists(tokens, lengths), self._lists(frames, lengths)
        times = []
        for pred, f in zip(preds, fr):
            items = []
            for k, t in zip(pred, f):                      # translate()'s walk: a list ends before its first EOS and skips PAD
                if k == BOS:
                    break
                if k != BLK:
                    items.append((self.idx2unit[k], t))
            times.append(items)
        return self.translate(preds), times
