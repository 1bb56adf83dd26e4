"""CTC segmentation of long recordings (Kuerzinger et al. 2020): where in minutes of audio each utterance of a known transcript lies,
and how far to trust it.  The CTC head's log-probs of the whole recording come from overlapping windows run as one batch
(window_plan says which encoder frames of which window are kept); ops.ctc_segment (include/otrans_hip.h otr_ctc_segment) then aligns
the concatenated transcript with free ends in one launch."""
import torch

from . import ops


def window_plan(T, window, hop):
    """Cut T feature frames into windows of `window` frames that start every `hop` frames (hop a multiple of 4, window >= hop + 8; the
    last window is the shorter rest).  The frontend's two stride-2 convolutions see 7 feature frames from 4k on for encoder frame k
    (ops.conv_geometry), so encoder frame k of window i is global encoder frame i * hop / 4 + k.  Of each inner window the central
    hop / 4 frames are kept, of the first everything up to there, of the last everything from there on: every global frame in
    [0, T2(T)) is produced exactly once.  Returns a list of (start, length, lo, hi, out) per window: features[start:start + length]
    go in, encoder frames [lo, hi) of its output are global frames [out, out + hi - lo)."""
    T, window, hop = int(T), int(window), int(hop)
    if hop < 4 or hop % 4 != 0:
        raise ValueError('window_plan: hop=%d must be a positive multiple of 4 (the frontend\'s subsampling)' % hop)
    if window < hop + 8:
        raise ValueError('window_plan: window=%d must be >= hop + 8 = %d' % (window, hop + 8))
    t2 = lambda n: ops.conv_geometry(n, 1)[2]    # noqa: E731
    total = t2(T)
    if T < 7 or total < 1:
        raise ValueError('window_plan: %d feature frames give no encoder frame' % T)
    n_win = 1 if T <= window else -(-(T - window) // hop) + 1
    q = hop // 4
    c = (t2(window) - q) // 2                    # the kept centre of an inner window is [c, c + q)
    plan = []
    for i in range(n_win):
        start = i * hop
        length = min(window, T - start)
        lo = 0 if i == 0 else c
        hi = t2(length) if i == n_win - 1 else c + q
        plan.append((start, length, lo, hi, i * q + lo))
    assert plan[-1][4] + plan[-1][3] - plan[-1][2] == total
    return plan


class CTCSegmenter:
    """Segments one long recording against its transcript.  `model` is anything with frontend / encoder / assistor (like
    recognize.CTCRecognizer's).  window / hop: feature frames, as window_plan takes them.  skip_logp <= 0: what a frame outside the
    path costs (otr_ctc_segment says why 0 shrinks the first and last label and what ln 0.5 does).  conf_window: labels per window
    of the confidence."""

    def __init__(self, model, window=1600, hop=800, skip_logp=0.0, conf_window=8):
        window_plan(window, window, hop)         # refuses a bad pair here, not at the first recording
        if conf_window < 1:
            raise ValueError('CTCSegmenter: conf_window=%d must be >= 1' % conf_window)
        self.model = model.eval()
        self.window, self.hop, self.skip_logp, self.conf_window = int(window), int(hop), float(skip_logp), int(conf_window)

    @torch.no_grad()
    def log_probs(self, features):
        """features f32 [T, F] of one recording -> the CTC head's log-probs f32 [T', V], T' = T2(T): all windows as one masked batch
        through the frontend, the encoder and assistor.inference, the kept frames of each stitched together"""
        if features.dim() != 2:
            raise ValueError('CTCSegmenter: features must be [T, F], got %s' % (tuple(features.shape),))
        T, F = features.shape
        plan = window_plan(T, self.window, self.hop)
        width = max(length for _, length, _, _, _ in plan)
        x = features.new_zeros((len(plan), width, F))
        mask = torch.zeros((len(plan), width), dtype=torch.bool, device=features.device)
        for i, (start, length, _, _, _) in enumerate(plan):
            x[i, :length] = features[start:start + length]
            mask[i, :length] = True
        fx, fm, _ = self.model.frontend.inference(x, mask, None)
        memory, memory_mask, _ = self.model.encoder(fx, fm)
        lp, _ = self.model.assistor.inference(memory, memory_mask)
        return torch.cat([lp[i, lo:hi] for i, (_, _, lo, hi, _) in enumerate(plan)], dim=0).float().contiguous()

    @torch.no_grad()
    def segment(self, features, utterances):
        """utterances: a list of non-empty lists of unit ids (no BOS / EOS), in the order they are spoken, at most
        ops.CTC_SEGMENT_MAX_TGT labels in all (a longer transcript is the caller's loop over chapters).  One ops.ctc_segment call with
        free ends.  Returns one (start_frame, end_frame, confidence, [(unit_id, start, end, logp), ...]) per utterance: start_frame is
        the first encoder frame of its first label, end_frame one past the last frame of its last label
        (recognize.frames_to_seconds turns them into times).  confidence: with m_j = logp_j / (end_j - start_j) the minimum, over every
        window of min(conf_window, n) consecutive labels of the utterance, of the mean of m_j.  A recording that cannot be segmented
        gives None for every utterance."""
        lengths = [len(u) for u in utterances]
        if not lengths or min(lengths) < 1:
            raise ValueError('CTCSegmenter.segment: every utterance needs at least one label')
        n = sum(lengths)
        if n > ops.CTC_SEGMENT_MAX_TGT:
            raise ValueError('CTCSegmenter.segment: a transcript of %d labels, one call takes at most %d'
                             % (n, ops.CTC_SEGMENT_MAX_TGT))
        lp = self.log_probs(features)
        dev = lp.device
        labels = torch.tensor([[int(c) for u in utterances for c in u]], dtype=torch.int64, device=dev)
        _, spans, label_logp, score, _ = ops.ctc_segment(
            lp.unsqueeze(0), torch.tensor([lp.shape[0]], dtype=torch.int32, device=dev), labels,
            torch.tensor([n], dtype=torch.int32, device=dev), blank=self.model.assistor.blank, free_start=True, free_end=True,
            skip_logp=self.skip_logp)
        if not float(score[0]) > -float('inf'):      # infeasible: the spans are -1, there is nothing to rate
            return [None] * len(utterances)
        m = label_logp[0] / (spans[0, :, 1] - spans[0, :, 0]).to(torch.float32)
        conf, at = [], 0
        for k in lengths:
            conf.append(m[at:at + k].unfold(0, min(self.conf_window, k), 1).mean(-1).min())
            at += k
        conf, spans, label_logp = torch.stack(conf).cpu(), spans[0].cpu(), label_logp[0].cpu()
        out, at = [], 0
        for u, k in enumerate(lengths):
            items = [(int(c), int(spans[at + j, 0]), int(spans[at + j, 1]), float(label_logp[at + j])) for j, c in enumerate(utterances[u])]
            out.append((items[0][1], items[-1][2], float(conf[u]), items))
            at += k
        return out
