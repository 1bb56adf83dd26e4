"""Plain-numpy restatement of what the otr_lstm_* kernels compute (include/otrans_hip.h): one nn.LSTM layer's forward pass from the
zero state that keeps the gate activations and cell states, and backpropagation through time step by step.  Time-major: x [T, B, Hin].
float64 by default, so that it serves as the reference the device results are measured against."""
import numpy as np


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def cell_fwd(z, c_prev):
    """z [B, 4H] gate pre-activations (i | f | g | o), c_prev [B, H] or None -> (act [B, 4H], c, h)"""
    H = z.shape[1] // 4
    a = np.concatenate([sigmoid(z[:, :H]), sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), sigmoid(z[:, 3 * H:])], axis=1)
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    c = i * g if c_prev is None else f * c_prev + i * g
    return a, c, o * np.tanh(c)


def cell_bwd(dh, dc_next, a, c, c_prev):
    """otr_lstm_bwd_step's cell part: total dh [B, H], dc from step t+1 (or None), saved act / c_t / c_{t-1} (or None) -> (dG, dc_prev)"""
    H = c.shape[1]
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    tc = np.tanh(c)
    dc = dh * o * (1 - tc * tc) + (0 if dc_next is None else dc_next)
    cp = np.zeros_like(c) if c_prev is None else c_prev
    dG = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
    return dG, dc * f


def layer_fwd(x, w_ih, w_hh, b_ih, b_hh):
    """-> (h [T, B, H], saved = dict(act [T, B, 4H], c [T, B, H]))"""
    T, B, _ = x.shape
    H = w_hh.shape[1]
    gx = x @ w_ih.T + b_ih
    h = np.zeros((T, B, H), x.dtype)
    c = np.zeros((T, B, H), x.dtype)
    act = np.zeros((T, B, 4 * H), x.dtype)
    for t in range(T):
        z = gx[t] + b_hh + (h[t - 1] @ w_hh.T if t else 0)
        act[t], c[t], h[t] = cell_fwd(z, c[t - 1] if t else None)
    return h, dict(act=act, c=c)


def layer_bwd(dy, x, h, saved, w_ih, w_hh):
    """dy [T, B, H] = dL/dh_t from above -> (dx, dw_ih, dw_hh, db (= db_ih = db_hh), dG [T, B, 4H])"""
    T, B, H = dy.shape
    act, c = saved['act'], saved['c']
    dG = np.zeros((T, B, 4 * H), dy.dtype)
    dc = None
    for t in range(T - 1, -1, -1):
        dh = dy[t] + (dG[t + 1] @ w_hh if t < T - 1 else 0)
        dG[t], dc = cell_bwd(dh, dc, act[t], c[t], c[t - 1] if t else None)
    G2 = dG.reshape(T * B, 4 * H)
    dx = (G2 @ w_ih).reshape(x.shape)
    dw_ih = G2.T @ x.reshape(T * B, -1)
    dw_hh = dG[1:].reshape(-1, 4 * H).T @ h[:-1].reshape(-1, H) if T > 1 else np.zeros_like(w_hh)
    return dx, dw_ih, dw_hh, G2.sum(0), dG


def stack_fwd_bwd(x, layers, dy_top, masks=None):
    """several layers (list of (w_ih, w_hh, b_ih, b_hh)), masks[k] = the dropout multiplier applied to layer k's output before layer
    k+1 (None: none).  -> (h of the top layer, dx, [(dw_ih, dw_hh, db) per layer])"""
    xs, hs, saves = [], [], []
    inp = x
    for k, (wi, wh, bi, bh) in enumerate(layers):
        if k and masks is not None and masks[k - 1] is not None:
            inp = inp * masks[k - 1]
        xs.append(inp)
        h, s = layer_fwd(inp, wi, wh, bi, bh)
        hs.append(h)
        saves.append(s)
        inp = h
    grads = [None] * len(layers)
    d = dy_top
    for k in range(len(layers) - 1, -1, -1):
        wi, wh, _, _ = layers[k]
        dx, dwi, dwh, db, _ = layer_bwd(d, xs[k], hs[k], saves[k], wi, wh)
        grads[k] = (dwi, dwh, db)
        d = dx
        if k and masks is not None and masks[k - 1] is not None:
            d = d * masks[k - 1]
    return hs[-1], d, grads
