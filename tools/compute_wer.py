"""WER / CER of a prediction file against a target file, scored on the GPU (opentransformer_amd.evaluate.score_texts): the
equivalent of the reference's tools/computer_wer.py without the `editdistance` package.  Both files hold lines `utt_id unit unit ...`.
Every utterance of the prediction file is scored against the target of the same id; an id the target file lacks is an error (KeyError),
as in the reference.

    python tools/compute_wer.py target_file predict_file
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_units(path):
    """lines `utt_id unit unit ...` -> dict utt_id -> list of units, in file order (a repeated id keeps its last line)"""
    out = {}
    with open(path, 'r', encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split()
            if parts:
                out[parts[0]] = parts[1:]
    return out


def check_ids(targets, predictions):
    for utt in predictions:
        if utt not in targets:
            raise KeyError('%s: in the prediction file and not in the target file' % utt)


def report(res):
    return ('The WER/CER is %.2f\n' % res['wer']
            + '%d errors in %d units of %d utterances: %d substitutions, %d deletions, %d insertions'
            % (res['errors'], res['ref_tokens'], res['utterances'], res['substitutions'], res['deletions'], res['insertions']))


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    targets, predictions = read_units(argv[1]), read_units(argv[2])
    check_ids(targets, predictions)
    from opentransformer_amd.evaluate import score_texts
    print(report(score_texts(targets, predictions)))


if __name__ == '__main__':
    main(sys.argv)
