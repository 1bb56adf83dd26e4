"""What every wrapper over the C ABI needs and nothing else: the process state, the kernel-timing hook, the device check, torch's
current stream, a tensor's address and a lengths vector in the ABI's form.  ops.py imports these back under the same names; a leaf
module (decode_ops.py, data_ops.py) imports this module and never ops."""
import ctypes as C

import torch

from . import _lib as L

_state = {'compute': 'bf16', 'rng_offset': 0, 'seed': None}      # only ever mutated in place: ops._state is this dict


# ---------------------------------------------------------------------------------------- kernel timing hook (bench.py)
# bench.py's `roofline` times the dominant kernels INSIDE a real training step: with a timer installed the wrappers of
# the hot launches bracket them with events on the launch stream (torch's current stream is the stream handed to the
# library).  Off (None) in production: one dict lookup per launch.
def set_kernel_timer(records):
    """records: a list that receives (name, meta, start_event, end_event) tuples, or None to switch timing off"""
    _state['ktimer'] = records


def _timed(name, meta, call):
    rec = _state.get('ktimer')
    if rec is None:
        return call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = call()
    e1.record()
    rec.append((name, meta, e0, e1, call))
    return r


def _cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.OtransHipError('opentransformer_amd ops need CUDA/HIP tensors (got a %s tensor); '
                                   'there is no CPU fallback' % t.device)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, offset_elems=0):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _len32(t):
    """a vector of lengths as the entries take it: flat, int32, contiguous"""
    return t.reshape(-1).to(torch.int32).contiguous()
