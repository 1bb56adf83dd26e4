"""Estimate a character n-gram LM from transcripts on the GPU (opentransformer_amd.ngram.NGramLM.train: interpolated modified
Kneser-Ney) and write it as ARPA text: the file NGramLM.from_arpa, CTCRecognizer(ngram_lm=...) and SpeechToTextRecognizer(ngram_lm=...)
start from.

    python tools/train_ngram.py TEXT VOCAB --order 3 -o lm.arpa[.gz]

TEXT holds lines `utt_id unit unit ...` (with --no-ids: bare `unit unit ...` lines); VOCAB is the vocabulary file of training, lines
`unit idx`.  A unit the vocabulary lacks maps to <UNK> if the vocabulary has it; otherwise the sentence is skipped and counted.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

UNK = '<UNK>'


def read_vocab(path):
    """lines `unit idx` -> dict unit -> idx"""
    unit2idx = {}
    with open(path, 'r', encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split()
            if parts:
                unit2idx[parts[0]] = int(parts[1])
    return unit2idx


def read_sentences(path, unit2idx, ids=True, eos_unit=1):
    """-> (list of id lists, number of skipped sentences, number of units mapped to <UNK>); a sentence that names a unit the
    estimator refuses inside a sentence (id 0, the </s> unit) is skipped as well"""
    unk = unit2idx.get(UNK)
    sents, skipped, mapped = [], 0, 0
    with open(path, 'r', encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split()
            if not parts:
                continue
            units = parts[1:] if ids else parts
            row = [unit2idx.get(u, unk) for u in units]
            if None in row or any(v < 1 or v == eos_unit for v in row):
                skipped += 1
                continue
            mapped += sum(u not in unit2idx for u in units)
            sents.append(row)
    return sents, skipped, mapped


def train_file(text, vocab, out, order=3, ids=True, eos_unit=1, device='cuda'):
    """the command as a function: returns (the NGramLM, the report dict)"""
    from opentransformer_amd.ngram import NGramLM
    unit2idx = read_vocab(vocab)
    idx2unit = {i: u for u, i in unit2idx.items()}
    sents, skipped, mapped = read_sentences(text, unit2idx, ids, eos_unit)
    units = sorted({i for i in idx2unit if i >= 1} | {eos_unit})          # the predictable units: the vocabulary's ids, not its gaps
    lm = NGramLM.train(sents, order=order, vocab_size=max(idx2unit) + 1, units=units, eos_unit=eos_unit, device=device)
    lm.to_arpa(out, idx2unit, eos_unit=eos_unit)
    rep = dict(sentences=lm.stats['sentences'], tokens=lm.stats['tokens'], skipped=skipped, unk=mapped, ngrams=lm.stats['ngrams'],
               discounts=lm.stats['discounts'], fallback_orders=lm.stats['fallback_orders'])
    return lm, rep


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('text')
    ap.add_argument('vocab')
    ap.add_argument('--order', type=int, default=3)
    ap.add_argument('-o', '--output', required=True)
    ap.add_argument('--no-ids', action='store_true', help='TEXT lines do not start with an utterance id')
    ap.add_argument('--eos', type=int, default=1, help='the unit id written as </s>')
    a = ap.parse_args(argv[1:])
    _, rep = train_file(a.text, a.vocab, a.output, order=a.order, ids=not a.no_ids, eos_unit=a.eos)
    print('%d sentences, %d units (%d skipped sentences, %d units mapped to %s)' % (rep['sentences'], rep['tokens'], rep['skipped'],
                                                                                 rep['unk'], UNK))
    print('n-grams per order: %s; discounts %s; orders on the fallback discounts: %s'
          % (rep['ngrams'], [tuple(round(v, 4) for v in d) for d in rep['discounts']], rep['fallback_orders'] or 'none'))
    print('wrote %s' % a.output)


if __name__ == '__main__':
    main(sys.argv)
