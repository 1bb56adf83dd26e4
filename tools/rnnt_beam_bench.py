"""The transducer's beam search, benchmark (ops.rnnt_beam, TransducerRecognizer(mode='beam'), csrc/rnntbeam.hip).  One JSON line, at the
model of tools/rnnt_bench.py part (c): the C2 encoder with an LSTM predictor (E 256, H 512, 2 layers) and joint 512 in fp16, B 32,
1000 frames, V 4233 -- per beam width W in (4, 10):
  decode_ms         recognize_tokens: frontend, encoder and the search
  search_ms         ops.rnnt_beam alone on the encoder projection, and per_frame_ms = search_ms / T'
  select_ms         the otr_rnnt_beam_select launch alone on logits [B * W, V] of that width with every slot live, against the time
                    of its own logits traffic (every row read W + 1 times by its wavefront, once from HBM: the floor counts it once)
                    at the 8 TB/s figure of DESIGN.md
  gather_ms         the otr_rnnt_beam_gather launch alone on the predictor's state table (h and c per layer, pg, the twins of h)
and the greedy decode of the same batch in the same run.  Warm-up, then timed repeats with device events; medians.

    python tools/rnnt_beam_bench.py [--iters 10] [--frames 1000] [--mode fp16] [--out profiles/rnnt_beam_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opentransformer_amd as ota                        # noqa: E402
from opentransformer_amd import _lib as L, ops, synthetic as syn          # noqa: E402

HBM_BYTES_PER_S = 8e12
B, J, U = 32, 512, 20
WIDTHS = (4, 10)
MAX_LEN = 100
DEV = 'cuda'


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def select_alone(W, V, iters):
    """the select launch on random logits, every slot live with its own history of 20 tokens (no merges: the compare of (b) runs
    its length check only, as in most frames of a real search)"""
    lib = L.load()
    R, ld = B * W, (V + 7) // 8 * 8
    g = torch.Generator(device=DEV).manual_seed(W)
    logits = torch.randn((R, ld), generator=g, device=DEV)
    score = -torch.rand((R,), generator=g, device=DEV)
    n = torch.full((R,), 20, dtype=torch.int32, device=DEV)
    tokens = torch.randint(1, V, (R, MAX_LEN), generator=g, device=DEV)
    frames = torch.zeros((R, MAX_LEN), dtype=torch.int32, device=DEV)
    el = torch.full((B,), 250, dtype=torch.int32, device=DEV)
    so, no, to, fo = torch.empty_like(score), torch.empty_like(n), torch.zeros_like(tokens), torch.zeros_like(frames)
    parent, emit = torch.empty_like(n), torch.empty_like(n)
    step_tok = torch.empty((R,), dtype=torch.int64, device=DEV)

    def run():
        L.check(lib.otr_rnnt_beam_select(_p(logits), ld, _p(el), B, W, 250, 100, V, 0, MAX_LEN, _p(score), _p(n), _p(tokens), _p(frames),
                                         _p(so), _p(no), _p(to), _p(fo), _p(parent), _p(step_tok), _p(emit), _stream()), 'otr_rnnt_beam_select')
    ms = timed(run, iters)
    floor = R * V * 4 / HBM_BYTES_PER_S * 1e3
    return {'select_ms': round(ms, 4), 'select_logits_mb': round(R * V * 4 / 1e6, 3), 'select_floor_ms': round(floor, 5),
            'select_over_floor': round(ms / floor, 1)}


def gather_alone(W, H, layers, half, iters):
    lib = L.load()
    R = B * W
    widths = [4 * H] * (2 * layers) + [4 * J] + ([2 * H] * layers if half else [])
    src = [torch.zeros((R, w // 4), dtype=torch.int32, device=DEV) for w in widths]
    dst = [torch.zeros((R, w // 4), dtype=torch.int32, device=DEV) for w in widths]
    parent = torch.randint(0, W, (R,), device=DEV).to(torch.int32)
    k = len(widths)
    sp, dp = (C.c_void_p * k)(*[x.data_ptr() for x in src]), (C.c_void_p * k)(*[x.data_ptr() for x in dst])
    nb = (C.c_int32 * k)(*widths)

    def run():
        L.check(lib.otr_rnnt_beam_gather(_p(parent), sp, dp, nb, k, B, W, _stream()), 'otr_rnnt_beam_gather')
    ms = timed(run, iters)
    traffic = 2 * R * sum(widths)
    return {'gather_ms': round(ms, 4), 'gather_items': k, 'gather_traffic_mb': round(traffic / 1e6, 3),
            'gather_over_floor': round(ms / (traffic / HBM_BYTES_PER_S * 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--mode', default='fp16', choices=['fp16', 'bf16', 'fp32'])
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'rnnt_beam_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rnnt_beam_bench needs a GPU')
    ops.set_compute_dtype(a.mode)
    cfg = syn.c2_model(0.1)
    V = cfg['decoder']['vocab_size']
    params = {k: v for k, v in cfg.items() if k not in ('decoder', 'decoder_type')}
    params.update(vocab_size=V, joint_size=J, predictor=dict(embedding_size=256, hidden_size=512, num_layers=2, dropout=0.1))
    model = ota.TransducerModel(params)
    syn.fill_state_dict_(model.state_dict(), 1234)
    model = model.to(DEV).eval()
    inputs, _ = syn.synthetic_batch(B, a.frames, 80, V, U, seed=0)
    x, m = inputs['inputs'].to(DEV), inputs['mask'].to(DEV)
    units = {i: str(i) for i in range(V)}
    res = {'shape': {'B': B, 'frames': a.frames, 'V': V, 'J': J, 'max_len': MAX_LEN}, 'mode': a.mode, 'iters': a.iters,
           'model': 'c2 encoder + LSTM predictor (E 256, H 512, 2 layers) + joint 512'}
    out = {}
    greedy = ota.TransducerRecognizer(model, units, max_symbols=4, max_len=MAX_LEN)

    def dec_greedy():
        out['g'] = greedy.recognize_tokens(x, m)
    res['greedy_decode_ms'] = round(timed(dec_greedy, a.iters), 3)
    res['greedy_mean_tokens'] = round(float(out['g'][1].float().mean()), 1)
    with torch.no_grad():
        pe, el = greedy._project(x, m)
    res['encoder_frames'] = int(pe.shape[1])

    def search_greedy():
        ops.rnnt_greedy(pe, el, model.predictor_step, model.joint.logits, max_symbols=4, max_len=MAX_LEN)
    res['greedy_search_ms'] = round(timed(search_greedy, a.iters), 3)
    for W in WIDTHS:
        rec = ota.TransducerRecognizer(model, units, max_len=MAX_LEN, mode='beam', beam_width=W, nbest=W)

        def decode():
            out['b'] = rec.recognize_tokens(x, m)

        def search():
            ops.rnnt_beam(pe, el, model.predictor_step, model.joint.logits, beam_width=W, max_len=MAX_LEN)
        r = {'decode_ms': round(timed(decode, a.iters), 3), 'search_ms': round(timed(search, a.iters), 3)}
        r['per_frame_ms'] = round(r['search_ms'] / pe.shape[1], 4)
        r['mean_tokens_1best'] = round(float(out['b'][1][:, 0].float().mean()), 1)
        r['live_slots'] = int((out['b'][2] > float('-inf')).sum())
        r['decode_over_greedy'] = round(r['decode_ms'] / res['greedy_decode_ms'], 2)
        r.update(select_alone(W, V, a.iters))
        r.update(gather_alone(W, 512, 2, a.mode != 'fp32', a.iters))
        res['W%d' % W] = r
    ops.set_compute_dtype('bf16')
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
