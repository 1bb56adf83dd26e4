"""GPU (-m gpu): evaluate.evaluate / recognize_tokens / score_texts.  The device tensors of recognize_tokens spell the strings
recognize() returns, for every recognizer and decode loop, and the error rates of evaluate() over two batches are those the
restatement (tests/edit_distance_ref.py) gives on the host for recognize()'s strings and the reference tokens.  Exact."""
import numpy as np
import pytest
import torch

from opentransformer_amd import evaluate
from opentransformer_amd import synthetic as syn
from tests import edit_distance_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 1234                             # of the weights: with it the n-best scores of every utterance are pairwise distinct (asserted)
PENALTY_KW = dict(penalty=0.6, lamda=5)
IDX2UNIT = {i: str(i) for i in range(100)}
RESCORE_MAX_LEN = 32
RECOGNIZERS = ['ctc_greedy', 'ctc_beam', 'att', 'att_cached', 'att_rescore']


@pytest.fixture(scope='module')
def setup():
    import opentransformer_amd as ota
    model = ota.SpeechToText(syn.c1_model(ctc_weight=0.3))
    syn.fill_state_dict_(model.state_dict(), SEED)
    model = model.to(DEV).eval()
    batches = []
    for seed, lengths, tgt in ((11, [120, 96, 57, 111], [6, 4, 5, 6]), (12, [118, 120, 83, 64], [3, 6, 6, 1])):
        inputs, targets = syn.synthetic_batch(batch=4, frames=120, feat_dim=80, vocab=100, tgt_len=6, seed=seed, lengths=lengths,
                                              tgt_lengths=tgt)
        batches.append((['utt%d_%d' % (seed, b) for b in range(4)], {k: v.to(DEV) for k, v in inputs.items()},
                        {k: v.to(DEV) for k, v in targets.items()}))
    return model, batches


def build(model, kind):
    from opentransformer_amd.recognize import CTCRecognizer, SpeechToTextRecognizer
    if kind == 'ctc_greedy':
        return CTCRecognizer(model, idx2unit=IDX2UNIT, mode='greedy')
    if kind == 'ctc_beam':
        return CTCRecognizer(model, idx2unit=IDX2UNIT, mode='beam', beam_width=5)
    # max_len 12 ends the step loops of a random-weight decoder.  rescore=True has no step loop: there max_len only bounds the hypotheses
    # that are rescored (one of more than max_len - 1 tokens scores -inf, and two of them tie).  A random-weight CTC head emits almost a
    # token per encoder frame, up to T' = 29 here, so at 12 the n-best scores could not be distinct; the rescoring recognizer gets
    # RESCORE_MAX_LEN >= T' + 1 = 30: every hypothesis of the search is rescored.
    kw = dict(idx2unit=IDX2UNIT, beam_width=5, nbest=3, max_len=RESCORE_MAX_LEN if kind == 'att_rescore' else 12, ctc_weight=0.3)
    return SpeechToTextRecognizer(model, apply_cache=kind == 'att_cached', rescore=kind == 'att_rescore', **kw)


def strings_and_scores(rec, kind, inputs):
    """recognize() as ([B][n] strings, scores [B, n] or None)"""
    out = rec.recognize(inputs['inputs'], inputs['mask'])
    if kind.startswith('ctc'):
        return [[s] for s in out], None
    return out[0], out[1]


@pytest.mark.parametrize('kind', RECOGNIZERS)
def test_recognize_tokens_and_evaluate(setup, kind):
    model, batches = setup
    rec = build(model, kind)
    want = np.zeros(8, np.int64)
    for _, inputs, targets in batches:
        strings, scores = strings_and_scores(rec, kind, inputs)
        tokens, lengths, tok_scores = rec.recognize_tokens(inputs['inputs'], inputs['mask'])
        n = len(strings[0])
        assert tokens.is_cuda and lengths.is_cuda and tok_scores.is_cuda
        assert tokens.dtype == torch.int64 and lengths.dtype == torch.int32 and tok_scores.dtype == torch.float32
        assert tokens.dim() == 3 and tokens.shape[:2] == (4, n) and lengths.shape == (4, n) and tok_scores.shape == (4, n)
        if scores is not None:
            # the precondition: the sorted n-best scores of every utterance are pairwise distinct (a device sort and the host sort may
            # order equal scores differently)
            for b in range(4):
                s = scores[b].tolist()
                assert all(s[i] > s[i + 1] for i in range(len(s) - 1)), (kind, b, s)
            assert torch.equal(tok_scores.cpu(), scores)
            assert rec.nbest_translate(tokens.cpu()) == strings
        # the lengths end every hypothesis where the strings end
        lens = lengths.cpu()
        if scores is None:
            assert [[rec.translate([tokens[b, 0, :int(lens[b, 0])].cpu()])[0]] for b in range(4)] == strings
        else:
            past = torch.arange(tokens.size(-1)).view(1, 1, -1) >= lens.unsqueeze(-1)
            assert rec.nbest_translate(tokens.cpu().masked_fill(past, 1)) == strings          # 1: EOS
            assert lens.tolist() == [[len(s.split()) for s in utt] for utt in strings]
        # the restatement on the host, from the strings alone
        hyps = [[[int(u) for u in s.split()] for s in utt] for utt in strings]
        Lh = max(1, max(len(h) for utt in hyps for h in utt))
        hyp = np.zeros((4, n, Lh), np.int64)
        hyp_len = np.zeros((4, n), np.int64)
        for b in range(4):
            for i in range(n):
                hyp[b, i, :len(hyps[b][i])] = hyps[b][i]
                hyp_len[b, i] = len(hyps[b][i])
        tg, tl = targets['targets'].cpu().numpy(), targets['targets_length'].cpu().numpy()
        want += ref.batch(tg[:, 1:], tl - 1, hyp, hyp_len)[2]
    got = evaluate.evaluate(rec, batches)
    assert got == evaluate.result_from_totals(want), (got, want)
    assert got['utterances'] == 8 and got['bad'] == 0 and got['ref_tokens'] == 37 and got['errors'] > 0
    assert got['topn_wer'] <= got['wer']
    meter = evaluate.ErrorRateMeter(DEV)                                    # a caller's meter goes on accumulating
    evaluate.evaluate(rec, batches[:1], meter)
    assert evaluate.evaluate(rec, batches[1:], meter) == got


@pytest.mark.parametrize('kind', ['att', 'att_cached'])
def test_recognize_tokens_with_length_penalty(setup, kind):
    """with a length penalty the normalised scores are formed on the device here and on the host in recognize(): the same order and the
    same hypotheses, the scores to float32 rounding, not bit for bit.  The bound: the device's pow is specified to 16 ulp (the OpenCL
    full-profile bound the ROCm device library documents), the host's to 1, and each side's division rounds once (0.5): 18 ulp, an ulp
    being at most 2^-23 of the value"""
    from opentransformer_amd.recognize import SpeechToTextRecognizer
    model, batches = setup
    rec = SpeechToTextRecognizer(model, idx2unit=IDX2UNIT, beam_width=5, nbest=3, max_len=12, ctc_weight=0.3,
                                 apply_cache=kind == 'att_cached', **PENALTY_KW)
    _, inputs, _ = batches[0]
    strings, scores = rec.recognize(inputs['inputs'], inputs['mask'])
    tokens, lengths, tok_scores = rec.recognize_tokens(inputs['inputs'], inputs['mask'])
    for b in range(4):
        s = scores[b].tolist()
        assert all(s[i] > s[i + 1] for i in range(len(s) - 1)), (kind, b, s)
    assert rec.nbest_translate(tokens.cpu()) == strings
    assert lengths.cpu().tolist() == [[len(s.split()) for s in utt] for utt in strings]
    got = tok_scores.cpu()
    assert bool((got[:, :-1] > got[:, 1:]).all())
    assert bool(((got - scores).abs() <= 18 * 2.0 ** -23 * scores.abs()).all()), (got, scores)


def test_score_texts():
    refs = {'u1': 'the cat sat on the mat'.split(), 'u2': ['hello'], 'u3': [], 'u4': 'a b c'.split()}
    hyps = {'u4': [], 'u1': 'the cat sit on mat'.split(), 'zz': ['lost'], 'u2': ['hello'], 'u3': ['uh']}
    res = evaluate.score_texts(refs, hyps)
    assert res.pop('unmatched') == ['zz']
    # u4: 3 deletions; u1: 1 substitution + 1 deletion; u2: exact; u3: 1 insertion
    assert res == {'wer': 60.0, 'topn_wer': 60.0, 'utterances': 4, 'ref_tokens': 10, 'errors': 6, 'substitutions': 1, 'deletions': 4,
                   'insertions': 1, 'errors_oracle': 6, 'bad': 0}
    assert evaluate.score_texts([['a', 'b']], [['a']])['errors'] == 1
    empty = evaluate.score_texts({}, {'x': ['a']})
    assert empty['unmatched'] == ['x'] and empty['utterances'] == 0 and np.isnan(empty['wer'])
