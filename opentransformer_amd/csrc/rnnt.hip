// The transducer (RNN-T): the joint's broadcast-add-tanh with its two reductions, the lattice loss with its gradient into the joint's
// logits, and the per-step kernels of the greedy decoder.  include/otrans_hip.h states the semantics.  f32 in both builds; the 16-bit
// build parameter only names the type of the joint's operand twin.  Every element offset is 64-bit: at [32, 250, 21, 4233] the logits
// hold 7.1e8 floats, 2.8 GB.
//  * rnnt_joint_fwd:  a workgroup per group of rows (b, t, u), a thread per four columns: z = tanh(pe[b,t,:] + pg[b,u,:]) inside the
//                     lengths, zeros outside (pe / pg are not read there), f32 and the 16-bit twin in the same pass.
//  * rnnt_joint_red:  dpe / dpg, one instantiation each: a workgroup per output row and 256 columns, its four waves take every fourth
//                     term of the sum and thread-own float4 partials meet in LDS in a fixed order.  dz and z are read twice (once per
//                     reduction), 16 bytes per lane and coalesced over J both times; nothing outside the lengths is read.
//  * rnnt_rows:       one WAVE per live row: an online max / sum over V (16-byte loads behind the row's own alignment peel: V = 4233 puts
//                     the rows on every 4-byte offset), leaves lse, lp[blank] and lp[label] in compact [B, T, U1] arrays.
//  * rnnt_lattice:    grid 2B: workgroup 2b sweeps alpha of utterance b, 2b + 1 its beta; one thread per column u, one barrier per
//                     anti-diagonal, the left / right neighbour's value through LDS, the two log-probs of the next diagonal fetched
//                     before the barrier.  It also takes the guard (lengths, then the labels) and writes nll and valid.
//  * rnnt_mean:       one workgroup: loss = (1 / B) sum nll through one fixed tree.
//  * rnnt_grad:       one wave per row of dlogits, live or not: the closed form of the header, or zeros.
//  * greedy_joint / greedy_advance / greedy_commit: one decode step's joint input, its arg-max + bookkeeping, and the row select that
//                     makes the candidate predictor state the committed one where a token was emitted.
#include "common.h"

#ifndef NEG_INF
#define NEG_INF (-__builtin_huge_valf())
#endif

constexpr int RN_COMMIT_ITEMS = 16;

__device__ __forceinline__ bool rn_len_ok(int Tb, int Ub, int T, int U1) {
  return Tb >= 1 && Tb <= T && Ub >= 0 && Ub < U1 && Ub <= OTR_RNNT_MAX_TGT;
}
__device__ __forceinline__ bool rn_label_ok(int64_t y, int V, int blank) { return y >= 0 && y < V && y != blank; }

// ---------------------------------------------------------------- joint
__global__ __launch_bounds__(256) void rnnt_joint_fwd_kernel(const float* pe, const float* pg, const int32_t* enc_len, const int32_t* tgt_len,
                                                             int T, int U1, int J, int64_t rows, int rpb, FastDiv dq, FastDiv du, FastDiv dt,
                                                             float* z, bf16_t* z16) {
  const int jq = J >> 2;
  const int n = rpb * jq;
  for (int i = threadIdx.x; i < n; i += 256) {
    const uint32_t r = fdiv((uint32_t)i, dq);
    const int64_t row = (int64_t)blockIdx.x * rpb + r;
    if (row >= rows) return;
    const int j4 = (i - (int)r * jq) * 4;
    const uint32_t bt = fdiv((uint32_t)row, du);
    const int u = (int)((uint32_t)row - bt * (uint32_t)U1);
    const uint32_t b = fdiv(bt, dt);
    const int t = (int)(bt - b * (uint32_t)T);
    const int Tb = min(max(enc_len[b], 0), T), Un = min(max(tgt_len[b] + 1, 0), U1);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < Tb && u < Un) {
      const float4 a = *reinterpret_cast<const float4*>(pe + (int64_t)bt * J + j4);
      const float4 g = *reinterpret_cast<const float4*>(pg + ((int64_t)b * U1 + u) * J + j4);
      o = make_float4(tanhf(a.x + g.x), tanhf(a.y + g.y), tanhf(a.z + g.z), tanhf(a.w + g.w));
    }
    *reinterpret_cast<float4*>(z + row * J + j4) = o;
    if (z16) *reinterpret_cast<uint2*>(z16 + row * J + j4) = make_uint2(pack2h(o.x, o.y), pack2h(o.z, o.w));
  }
}

// OVER_U: out[b, t, :] = sum over u < U_b + 1 (rows J apart); else out[b, u, :] = sum over t < T_b (rows U1 * J apart)
template <bool OVER_U>
__global__ __launch_bounds__(256) void rnnt_joint_red_kernel(const float* dz, const float* z, const int32_t* enc_len, const int32_t* tgt_len,
                                                             int T, int U1, int J, float* out) {
  __shared__ float4 part[4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane, idx = blockIdx.y, b = blockIdx.z;
  const int Tb = min(max(enc_len[b], 0), T), Un = min(max(tgt_len[b] + 1, 0), U1);
  int cnt;
  int64_t base, stride;
  if (OVER_U) {
    cnt = idx < Tb ? Un : 0;
    base = (((int64_t)b * T + idx) * U1) * J;
    stride = J;
  } else {
    cnt = idx < Un ? Tb : 0;
    base = (((int64_t)b * T) * U1 + idx) * J;
    stride = (int64_t)U1 * J;
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < (J >> 2)) {
    for (int i = sl; i < cnt; i += 4) {
      const int64_t o = base + i * stride + 4 * q;
      const float4 d = *reinterpret_cast<const float4*>(dz + o);
      const float4 y = *reinterpret_cast<const float4*>(z + o);
      acc.x += d.x * (1.f - y.x * y.x);
      acc.y += d.y * (1.f - y.y * y.y);
      acc.z += d.z * (1.f - y.z * y.z);
      acc.w += d.w * (1.f - y.w * y.w);
    }
  }
  part[sl][lane] = acc;
  __syncthreads();
  if (sl == 0 && q < (J >> 2)) {
    const float4 p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    const float4 s = make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z,
                                 ((p0.w + p1.w) + p2.w) + p3.w);
    const int64_t orow = OVER_U ? (int64_t)b * T + idx : (int64_t)b * U1 + idx;
    *reinterpret_cast<float4*>(out + orow * J + 4 * q) = s;
  }
}

// ---------------------------------------------------------------- loss: rows
struct RnRun { float m, s; };
__device__ __forceinline__ void rn_take(RnRun& r, float x) {
  if (x > r.m) {
    r.s = r.s * expf(r.m - x) + 1.f;
    r.m = x;
  } else if (x > NEG_INF) {
    r.s += expf(x - r.m);
  }
}
__device__ __forceinline__ void rn_take4(RnRun& r, const float4& q) {
  const float mq = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  if (mq > r.m) {
    r.s *= expf(r.m - mq);
    r.m = mq;
  }
  if (r.m > NEG_INF) r.s += (expf(q.x - r.m) + expf(q.y - r.m)) + (expf(q.z - r.m) + expf(q.w - r.m));
}
// floats in front of the first 16-byte boundary of a row (the row's own peel), at most n
__device__ __forceinline__ int rn_head(const float* x, int n) { return min((int)((4u - (uint32_t)(((uintptr_t)x >> 2) & 3u)) & 3u), n); }

__device__ __forceinline__ void rn_row(const float* x, int V, int lane, float& M, float& S) {
  RnRun r{NEG_INF, 0.f};
  const int head = rn_head(x, V);
  if (lane < head) rn_take(r, x[lane]);
  const float* xa = x + head;
  const int nq = (V - head) >> 2;
  int q = lane;
  for (; q + 192 < nq; q += 256) {                    // four loads in flight per lane
    const float4 a = *reinterpret_cast<const float4*>(xa + 4 * q);
    const float4 b = *reinterpret_cast<const float4*>(xa + 4 * (q + 64));
    const float4 c = *reinterpret_cast<const float4*>(xa + 4 * (q + 128));
    const float4 d = *reinterpret_cast<const float4*>(xa + 4 * (q + 192));
    rn_take4(r, a); rn_take4(r, b); rn_take4(r, c); rn_take4(r, d);
  }
  for (; q < nq; q += 64) rn_take4(r, *reinterpret_cast<const float4*>(xa + 4 * q));
  for (int v = head + 4 * nq + lane; v < V; v += 64) rn_take(r, x[v]);
  M = wave_max(r.m);
  S = wave_sum(r.m > NEG_INF ? r.s * expf(r.m - M) : 0.f);
}

__device__ __forceinline__ void rn_coords(int64_t row, int T, int U1, int& b, int& t, int& u) {
  const int64_t bt = row / U1;
  u = (int)(row - bt * U1);
  b = (int)(bt / T);
  t = (int)(bt - (int64_t)b * T);
}

__global__ __launch_bounds__(256) void rnnt_rows_kernel(const float* logits, int64_t ld, const int64_t* labels, int64_t ldl,
                                                        const int32_t* enc_len, const int32_t* tgt_len, int T, int U1, int V, int blank,
                                                        int64_t rows, float* lse, float* lpb, float* lpl) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  int b, t, u;
  rn_coords(row, T, U1, b, t, u);
  const int Tb = enc_len[b], Ub = tgt_len[b];
  if (!rn_len_ok(Tb, Ub, T, U1) || t >= Tb || u > Ub) return;       // not live: the row is not read
  const float* x = logits + row * ld;
  float M, S;
  rn_row(x, V, lane, M, S);
  if (lane == 0) {
    const float zz = M + logf(S);
    lse[row] = zz;
    lpb[row] = x[blank] - zz;
    float l = NEG_INF;
    if (u < Ub) {
      const int64_t y = labels[(int64_t)b * ldl + u];
      if (rn_label_ok(y, V, blank)) l = x[y] - zz;    // range-checked before it is an index; a bad label kills the utterance below
    }
    lpl[row] = l;
  }
}

// ---------------------------------------------------------------- loss: lattice
__device__ __forceinline__ float rn_lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + log1pf(expf(-fabsf(a - b)));
}

__global__ __launch_bounds__(256) void rnnt_lattice_kernel(const int64_t* labels, int64_t ldl, const int32_t* enc_len, const int32_t* tgt_len,
                                                           int T, int U1, int V, int blank, const float* lpb, const float* lpl, float* alpha,
                                                           float* beta, float* nll, int32_t* valid, float* shifted) {
  __shared__ float sh[2][258];
  __shared__ float s_red[256];
  __shared__ int s_cnt[256];
  __shared__ int s_bad;
  const int u = threadIdx.x;
  const int b = blockIdx.x >> 1;
  const bool back = blockIdx.x & 1;
  const int Tb = enc_len[b], Ub = tgt_len[b];
  const bool len_ok = rn_len_ok(Tb, Ub, T, U1);
  if (u == 0) s_bad = 0;
  __syncthreads();
  if (len_ok && u < Ub && !rn_label_ok(labels[(int64_t)b * ldl + u], V, blank)) s_bad = 1;
  __syncthreads();
  if (!len_ok || s_bad) {                             // guarded: no likelihood, no gradient (rnnt_grad reads valid)
    if (!back && u == 0) {
      nll[b] = 0.f;
      valid[b] = 0;
    }
    return;
  }
  const int64_t base = (int64_t)b * T * U1;
  const int D = Tb + Ub - 1;                          // the last anti-diagonal
  const bool col = u <= Ub;
  // The sweeps run on SHIFTED log-probs lp + c, c = -(the mean of lp_blank over up to 256 evenly spaced live cells): alpha'(t,u) =
  // alpha(t,u) + (t + u) c and beta'(t,u) = beta(t,u) + (D + 1 - t - u) c stay of the size of the paths' spread, where the plain ones
  // grow like (t + u) |lp| (2400 at T 250, U 20, V 4233: a float32 ulp of 2.4e-4 in every exponent of the gradient).  Any c gives the
  // same mathematics; both workgroups of an utterance form it with the same arithmetic.
  float c;
  {
    const int ncell = Tb * (Ub + 1), stride = max(1, ncell >> 8), idx = u * stride;
    float v = 0.f;
    int k = 0;
    if (idx < ncell) {
      const int tt = idx / (Ub + 1), uu = idx - tt * (Ub + 1);
      v = lpb[base + (int64_t)tt * U1 + uu];
      k = 1;
    }
    s_red[u] = v;
    s_cnt[u] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {               // one tree, the same order in both workgroups
      if (u < o) {
        s_red[u] += s_red[u + o];
        s_cnt[u] += s_cnt[u + o];
      }
      __syncthreads();
    }
    c = -s_red[0] / (float)s_cnt[0];
    if (!(fabsf(c) < 1e30f)) c = 0.f;
  }
  if (!back) {
    // alpha(t, u) = lae(alpha(t-1, u) + lp_blank(t-1, u), alpha(t, u-1) + lp_label(t, u-1)); `own` is this column's previous value
    float own = NEG_INF, cb = NEG_INF, cl = NEG_INF;
    for (int d = 0; d <= D; ++d) {
      const int t = d - u;
      float nb = NEG_INF, nl = NEG_INF;               // the next diagonal's two log-probs: in flight over the barrier
      if (col && t + 1 >= 0 && t + 1 < Tb) {
        if (t + 1 > 0) nb = lpb[base + (int64_t)t * U1 + u] + c;
        if (u > 0) nl = lpl[base + (int64_t)(t + 1) * U1 + u - 1] + c;
      }
      float v = NEG_INF;
      if (col && t >= 0 && t < Tb) {
        if (d == 0) {
          v = 0.f;
        } else {
          const float left = u > 0 ? sh[(d - 1) & 1][u - 1] + cl : NEG_INF;
          v = rn_lae(own + cb, left);
        }
        alpha[base + (int64_t)t * U1 + u] = v;
        own = v;
      }
      sh[d & 1][u] = v;
      __syncthreads();
      cb = nb;
      cl = nl;
    }
    if (u == Ub) {                                    // own = alpha'(T_b - 1, U_b)
      const float lnp = own + (lpb[base + (int64_t)(Tb - 1) * U1 + Ub] + c);      // ln P + (D + 1) c
      nll[b] = -(lnp - (float)(D + 1) * c);
      valid[b] = 1;
      shifted[2 * b] = lnp;                           // what rnnt_grad subtracts, and the shift it adds to lp
      shifted[2 * b + 1] = c;
    }
  } else {
    // beta(t, u) = lae(beta(t+1, u) + lp_blank(t, u), beta(t, u+1) + lp_label(t, u)), beta(T_b, U_b) := 0, beta(T_b, u < U_b) := -inf
    float own = (u == Ub) ? 0.f : NEG_INF, cb = NEG_INF, cl = NEG_INF;
    {
      const int t = D - u;
      if (col && t >= 0 && t < Tb) {
        cb = lpb[base + (int64_t)t * U1 + u] + c;
        if (u < Ub) cl = lpl[base + (int64_t)t * U1 + u] + c;
      }
    }
    for (int d = D; d >= 0; --d) {
      const int t = d - u;
      float nb = NEG_INF, nl = NEG_INF;
      if (col && t - 1 >= 0 && t - 1 < Tb) {
        nb = lpb[base + (int64_t)(t - 1) * U1 + u] + c;
        if (u < Ub) nl = lpl[base + (int64_t)(t - 1) * U1 + u] + c;
      }
      float v = NEG_INF;
      if (col && t >= 0 && t < Tb) {
        const float right = u < Ub ? sh[(d + 1) & 1][u + 1] + cl : NEG_INF;      // at d == D only u == U_b is live: nothing is read
        v = rn_lae(own + cb, right);
        beta[base + (int64_t)t * U1 + u] = v;
        own = v;
      }
      sh[d & 1][u] = v;
      __syncthreads();
      cb = nb;
      cl = nl;
    }
  }
}

__global__ __launch_bounds__(256) void rnnt_mean_kernel(const float* nll, int B, float* loss) {
  __shared__ float s[256];
  float a = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) a += nll[b];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                 // one tree, the same order on every run
    if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = s[0] / (float)B;
}

// ---------------------------------------------------------------- loss: gradient
__device__ __forceinline__ float rn_g(float x, int v, float zz, float c0, int blank, float cb, int y, float cl) {
  return c0 * expf(x - zz) - (v == blank ? cb : 0.f) - (v == y ? cl : 0.f);
}

__global__ __launch_bounds__(256) void rnnt_grad_kernel(const float* logits, int64_t ld, const int64_t* labels, int64_t ldl,
                                                        const int32_t* enc_len, const int32_t* tgt_len, int B, int T, int U1, int V, int blank,
                                                        int64_t rows, const float* lse, const float* lpb, const float* lpl,
                                                        const float* alpha, const float* beta, const float* shifted, const int32_t* valid,
                                                        const float* grad_scale, float* dlogits, int64_t ldd) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  int b, t, u;
  rn_coords(row, T, U1, b, t, u);
  float* d = dlogits + row * ldd;
  const int W = (int)ldd;
  const int Tb = enc_len[b], Ub = tgt_len[b];
  if (!valid[b] || t >= Tb || u > Ub) {               // valid implies the lengths are in range: zeros, the logits are not read
    const int head = rn_head(d, W);
    if (lane < head) d[lane] = 0.f;
    float* da = d + head;
    const int nq = (W - head) >> 2;
    for (int q = lane; q < nq; q += 64) *reinterpret_cast<float4*>(da + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int v = head + 4 * nq + lane; v < W; v += 64) d[v] = 0.f;
    return;
  }
  const float s = (grad_scale ? *grad_scale : 1.f) / (float)B;
  const float lnP = shifted[2 * b], c = shifted[2 * b + 1], a = alpha[row], zz = lse[row];      // all three shifted alike (rnnt_lattice)
  const float bn = (t + 1 < Tb) ? beta[row + U1] : (u == Ub ? 0.f : NEG_INF);
  const float c0 = s * expf(a + beta[row] - lnP);
  const float cb = s * expf(a + (lpb[row] + c) + bn - lnP);
  int y = -1;
  float cl = 0.f;
  if (u < Ub) {
    y = (int)labels[(int64_t)b * ldl + u];            // inside [0, V): the utterance is valid
    cl = s * expf(a + (lpl[row] + c) + beta[row + 1] - lnP);
  }
  const float* x = logits + row * ld;
  if ((((uintptr_t)x ^ (uintptr_t)d) & 15) == 0) {    // both rows share one peel: 16-byte loads and stores
    const int head = rn_head(x, V);
    if (lane < head) d[lane] = rn_g(x[lane], lane, zz, c0, blank, cb, y, cl);
    const float* xa = x + head;
    float* da = d + head;
    const int nq = (V - head) >> 2;
    for (int q = lane; q < nq; q += 64) {
      const float4 in = *reinterpret_cast<const float4*>(xa + 4 * q);
      const int v = head + 4 * q;
      *reinterpret_cast<float4*>(da + 4 * q) = make_float4(rn_g(in.x, v, zz, c0, blank, cb, y, cl), rn_g(in.y, v + 1, zz, c0, blank, cb, y, cl),
                                                           rn_g(in.z, v + 2, zz, c0, blank, cb, y, cl), rn_g(in.w, v + 3, zz, c0, blank, cb, y, cl));
    }
    for (int v = head + 4 * nq + lane; v < V; v += 64) d[v] = rn_g(x[v], v, zz, c0, blank, cb, y, cl);
  } else {
    for (int v = lane; v < V; v += 64) d[v] = rn_g(x[v], v, zz, c0, blank, cb, y, cl);
  }
  for (int v = V + lane; v < W; v += 64) d[v] = 0.f;  // the padding behind the vocabulary
}

// ---------------------------------------------------------------- greedy decoding
__global__ __launch_bounds__(256) void rnnt_greedy_joint_kernel(const float* pe, const float* pg, const int32_t* tpos, const int32_t* nout,
                                                                const int32_t* enc_len, int T, int J, int max_len, float* z, bf16_t* z16) {
  const int b = blockIdx.x;
  const int Tb = min(max(enc_len[b], 0), T), t = tpos[b];
  const bool live = t >= 0 && t < Tb && nout[b] < max_len;
  for (int q = threadIdx.x; q < (J >> 2); q += 256) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 a = *reinterpret_cast<const float4*>(pe + ((int64_t)b * T + t) * J + 4 * q);
      const float4 g = *reinterpret_cast<const float4*>(pg + (int64_t)b * J + 4 * q);
      o = make_float4(tanhf(a.x + g.x), tanhf(a.y + g.y), tanhf(a.z + g.z), tanhf(a.w + g.w));
    }
    *reinterpret_cast<float4*>(z + (int64_t)b * J + 4 * q) = o;
    if (z16) *reinterpret_cast<uint2*>(z16 + (int64_t)b * J + 4 * q) = make_uint2(pack2h(o.x, o.y), pack2h(o.z, o.w));
  }
}

__global__ __launch_bounds__(256) void rnnt_greedy_advance_kernel(const float* logits, int64_t ld, const int32_t* enc_len, int T, int V, int blank,
                                                                  int max_symbols, int max_len, int32_t* tpos, int32_t* nout, int32_t* cnt,
                                                                  int64_t* tokens, int32_t* frames, float* score, int32_t* emit,
                                                                  int64_t* step_tok, int32_t* remaining) {
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  __shared__ float s_s[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int Tb = min(max(enc_len[b], 0), T);
  const int t = tpos[b], n = nout[b];
  if (t >= Tb || n >= max_len) {                      // done before this step: nothing moves
    if (tid == 0) {
      emit[b] = 0;
      step_tok[b] = blank;
    }
    return;
  }
  const float* x = logits + (int64_t)b * ld;
  float bv = NEG_INF;
  int bi = V;
  for (int v = tid; v < V; v += 256) {                // ascending per thread: > keeps the lowest index
    const float xv = x[v];
    if (xv > bv || bi == V) {
      bv = xv;
      bi = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    s_v[wid] = bv;
    s_i[wid] = bi;
  }
  __syncthreads();
  bv = s_v[0];
  bi = s_i[0];
  for (int w = 1; w < 4; ++w)
    if (s_v[w] > bv || (s_v[w] == bv && s_i[w] < bi)) {
      bv = s_v[w];
      bi = s_i[w];
    }
  float se = 0.f;
  for (int v = tid; v < V; v += 256) se += expf(x[v] - bv);
  se = wave_sum(se);
  if (lane == 0) s_s[wid] = se;
  __syncthreads();
  if (tid != 0) return;
  const float zz = bv + logf(((s_s[0] + s_s[1]) + s_s[2]) + s_s[3]);
  const int c = cnt[b];
  int t1 = t, n1 = n;
  if (bi != blank && bi < V && c < max_symbols) {
    tokens[(int64_t)b * max_len + n] = bi;
    frames[(int64_t)b * max_len + n] = t;
    score[b] += bv - zz;
    n1 = n + 1;
    nout[b] = n1;
    cnt[b] = c + 1;
    emit[b] = 1;
    step_tok[b] = bi;
  } else {
    t1 = t + 1;
    tpos[b] = t1;
    cnt[b] = 0;
    score[b] += x[blank] - zz;
    emit[b] = 0;
    step_tok[b] = blank;
  }
  if (t1 >= Tb || n1 >= max_len) atomicSub(remaining, 1);   // this row's one transition to done
}

struct RnCommit {
  const void* src[RN_COMMIT_ITEMS];
  void* dst[RN_COMMIT_ITEMS];
  int32_t words[RN_COMMIT_ITEMS];                     // 4-byte words per row
};
__global__ __launch_bounds__(256) void rnnt_greedy_commit_kernel(const int32_t* emit, RnCommit c) {
  const int b = blockIdx.x, k = blockIdx.y;
  if (!emit[b]) return;
  const int w = c.words[k];
  const uint32_t* s = (const uint32_t*)c.src[k] + (int64_t)b * w;
  uint32_t* d = (uint32_t*)c.dst[k] + (int64_t)b * w;
  for (int i = threadIdx.x; i < w; i += 256) d[i] = s[i];
}

// ---------------------------------------------------------------- entries
static bool rnnt_shape_ok(int64_t B, int64_t T, int64_t U1) {
  return B >= 1 && B <= 65535 && T >= 1 && T <= 65535 && U1 >= 1 && U1 <= OTR_RNNT_MAX_TGT + 1 && B * T * U1 < (1ll << 31) - 4;
}

extern "C" int32_t otr_rnnt_joint_fwd(const float* pe, const float* pg, const int32_t* enc_len, const int32_t* tgt_len, int32_t B, int32_t T,
                                      int32_t U1, int32_t J, float* z, void* z16, void* stream) {
  OTR_REQUIRE(rnnt_shape_ok(B, T, U1), "rnnt_joint_fwd: bad shape B=%d T=%d U1=%d (B, T <= 65535, U1 <= %d, B*T*U1 < 2^31)", B, T, U1,
              OTR_RNNT_MAX_TGT + 1);
  OTR_REQUIRE(J >= 4 && J % 4 == 0 && J <= 65536, "rnnt_joint_fwd: J=%d must be a multiple of 4 in [4, 65536]", J);
  OTR_REQUIRE(pe && pg && enc_len && tgt_len && z, "rnnt_joint_fwd: null pointer");
  OTR_REQUIRE(((uintptr_t)pe | (uintptr_t)pg | (uintptr_t)z) % 16 == 0 && (uintptr_t)z16 % 8 == 0, "rnnt_joint_fwd: pe, pg, z must be 16-byte aligned");
  const int64_t rows = (int64_t)B * T * U1;
  const int jq = J / 4;
  const int rpb = jq >= 1024 ? 1 : 1024 / jq;
  hipLaunchKernelGGL(rnnt_joint_fwd_kernel, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, (hipStream_t)stream, pe, pg, enc_len, tgt_len,
                     T, U1, J, rows, rpb, make_fastdiv(jq), make_fastdiv(U1), make_fastdiv(T), z, (bf16_t*)z16);
  return otr_check_launch("rnnt_joint_fwd");
}

extern "C" int32_t otr_rnnt_joint_bwd(const float* dz, const float* z, const int32_t* enc_len, const int32_t* tgt_len, int32_t B, int32_t T,
                                      int32_t U1, int32_t J, float* dpe, float* dpg, void* stream) {
  OTR_REQUIRE(rnnt_shape_ok(B, T, U1), "rnnt_joint_bwd: bad shape B=%d T=%d U1=%d (B, T <= 65535, U1 <= %d, B*T*U1 < 2^31)", B, T, U1,
              OTR_RNNT_MAX_TGT + 1);
  OTR_REQUIRE(J >= 4 && J % 4 == 0 && J <= 65536, "rnnt_joint_bwd: J=%d must be a multiple of 4 in [4, 65536]", J);
  OTR_REQUIRE(dz && z && enc_len && tgt_len && dpe && dpg, "rnnt_joint_bwd: null pointer");
  OTR_REQUIRE(((uintptr_t)dz | (uintptr_t)z | (uintptr_t)dpe | (uintptr_t)dpg) % 16 == 0, "rnnt_joint_bwd: dz, z, dpe, dpg must be 16-byte aligned");
  const unsigned gx = (unsigned)((J / 4 + 63) / 64);
  hipLaunchKernelGGL(rnnt_joint_red_kernel<true>, dim3(gx, T, B), dim3(256), 0, (hipStream_t)stream, dz, z, enc_len, tgt_len, T, U1, J, dpe);
  hipLaunchKernelGGL(rnnt_joint_red_kernel<false>, dim3(gx, U1, B), dim3(256), 0, (hipStream_t)stream, dz, z, enc_len, tgt_len, T, U1, J, dpg);
  return otr_check_launch("rnnt_joint_bwd");
}

extern "C" int64_t otr_rnnt_workspace_floats(int32_t B, int32_t T, int32_t U1) {
  if (!rnnt_shape_ok(B, T, U1)) return -1;
  return 5 * (int64_t)B * T * U1 + 2 * (int64_t)B;    // lse, lp_blank, lp_label, alpha, beta; per utterance the shifted ln P and the shift
}

extern "C" int32_t otr_rnnt_loss(const float* logits, int64_t ld, const int64_t* labels, int64_t ldl, const int32_t* enc_len,
                                 const int32_t* tgt_len, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, const float* grad_scale,
                                 float* loss, float* nll, int32_t* valid, float* dlogits, int64_t ldd, float* workspace,
                                 int64_t workspace_floats, void* stream) {
  OTR_REQUIRE(rnnt_shape_ok(B, T, U1), "rnnt_loss: bad shape B=%d T=%d U1=%d (B, T <= 65535, U1 <= %d, B*T*U1 < 2^31)", B, T, U1,
              OTR_RNNT_MAX_TGT + 1);
  OTR_REQUIRE(V >= 2 && ld >= V, "rnnt_loss: V=%d must be >= 2 and ld=%lld >= V", V, (long long)ld);
  OTR_REQUIRE(blank >= 0 && blank < V, "rnnt_loss: blank=%d outside [0, V=%d)", blank, V);
  OTR_REQUIRE(ldl >= U1 - 1 && ldl >= 0, "rnnt_loss: label row stride ldl=%lld < U1 - 1 = %d", (long long)ldl, U1 - 1);
  OTR_REQUIRE(logits && enc_len && tgt_len && loss && nll && valid && (labels || U1 == 1), "rnnt_loss: null pointer");
  OTR_REQUIRE(!dlogits || (ldd >= V && ldd < (1ll << 31)), "rnnt_loss: ld_dlogits=%lld < V=%d", (long long)ldd, V);
  const int64_t rows = (int64_t)B * T * U1;
  OTR_REQUIRE(workspace && workspace_floats >= 5 * rows + 2 * (int64_t)B, "rnnt_loss: workspace of %lld floats, %lld needed", (long long)workspace_floats,
              (long long)(5 * rows + 2 * (int64_t)B));
  float *lse = workspace, *lpb = lse + rows, *lpl = lpb + rows, *alpha = lpl + rows, *beta = alpha + rows, *shifted = beta + rows;
  hipStream_t s = (hipStream_t)stream;
  const unsigned gr = (unsigned)((rows + 3) / 4);
  hipLaunchKernelGGL(rnnt_rows_kernel, dim3(gr), dim3(256), 0, s, logits, ld, labels, ldl, enc_len, tgt_len, T, U1, V, blank, rows, lse, lpb, lpl);
  hipLaunchKernelGGL(rnnt_lattice_kernel, dim3(2 * (unsigned)B), dim3(256), 0, s, labels, ldl, enc_len, tgt_len, T, U1, V, blank,
                     (const float*)lpb, (const float*)lpl, alpha, beta, nll, valid, shifted);
  hipLaunchKernelGGL(rnnt_mean_kernel, dim3(1), dim3(256), 0, s, (const float*)nll, B, loss);
  if (dlogits)
    hipLaunchKernelGGL(rnnt_grad_kernel, dim3(gr), dim3(256), 0, s, logits, ld, labels, ldl, enc_len, tgt_len, B, T, U1, V, blank, rows,
                       (const float*)lse, (const float*)lpb, (const float*)lpl, (const float*)alpha, (const float*)beta, (const float*)shifted,
                       (const int32_t*)valid, grad_scale, dlogits, ldd);
  return otr_check_launch("rnnt_loss");
}

extern "C" int32_t otr_rnnt_greedy_joint(const float* pe, const float* pg_cur, const int32_t* t, const int32_t* n, const int32_t* enc_len,
                                         int32_t B, int32_t T, int32_t J, int32_t max_len, float* z, void* z16, void* stream) {
  OTR_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "rnnt_greedy_joint: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(J >= 4 && J % 4 == 0, "rnnt_greedy_joint: J=%d must be a positive multiple of 4", J);
  OTR_REQUIRE(pe && pg_cur && t && n && enc_len && z, "rnnt_greedy_joint: null pointer");
  OTR_REQUIRE(((uintptr_t)pe | (uintptr_t)pg_cur | (uintptr_t)z) % 16 == 0 && (uintptr_t)z16 % 8 == 0,
              "rnnt_greedy_joint: pe, pg_cur, z must be 16-byte aligned");
  hipLaunchKernelGGL(rnnt_greedy_joint_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pe, pg_cur, t, n, enc_len, T, J, max_len, z,
                     (bf16_t*)z16);
  return otr_check_launch("rnnt_greedy_joint");
}

extern "C" int32_t otr_rnnt_greedy_advance(const float* logits, int64_t ld, const int32_t* enc_len, int32_t B, int32_t T, int32_t V, int32_t blank,
                                           int32_t max_symbols, int32_t max_len, int32_t* t, int32_t* n, int32_t* count, int64_t* tokens,
                                           int32_t* frames, float* score, int32_t* emit, int64_t* step_tok, int32_t* remaining, void* stream) {
  OTR_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "rnnt_greedy_advance: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(V >= 2 && ld >= V && blank >= 0 && blank < V, "rnnt_greedy_advance: V=%d >= 2, ld=%lld >= V, blank=%d in [0, V) expected", V,
              (long long)ld, blank);
  OTR_REQUIRE(max_symbols >= 1 && max_len >= 1, "rnnt_greedy_advance: max_symbols=%d and max_len=%d must be >= 1", max_symbols, max_len);
  OTR_REQUIRE(logits && enc_len && t && n && count && tokens && frames && score && emit && step_tok && remaining,
              "rnnt_greedy_advance: null pointer");
  hipLaunchKernelGGL(rnnt_greedy_advance_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ld, enc_len, T, V, blank, max_symbols,
                     max_len, t, n, count, tokens, frames, score, emit, step_tok, remaining);
  return otr_check_launch("rnnt_greedy_advance");
}

extern "C" int32_t otr_rnnt_greedy_commit(const int32_t* emit, const void* const* src, void* const* dst, const int32_t* row_bytes,
                                          int32_t n_items, int32_t B, void* stream) {
  OTR_REQUIRE(B >= 1 && B <= 65535 && n_items >= 1 && n_items <= RN_COMMIT_ITEMS, "rnnt_greedy_commit: B=%d, n_items=%d (1 .. %d) not supported",
              B, n_items, RN_COMMIT_ITEMS);
  OTR_REQUIRE(emit && src && dst && row_bytes, "rnnt_greedy_commit: null pointer");
  RnCommit c;
  for (int k = 0; k < RN_COMMIT_ITEMS; ++k) {
    const int j = k < n_items ? k : 0;
    OTR_REQUIRE(src[j] && dst[j] && src[j] != dst[j] && row_bytes[j] > 0 && row_bytes[j] % 4 == 0 &&
                    ((uintptr_t)src[j] | (uintptr_t)dst[j]) % 4 == 0,
                "rnnt_greedy_commit: item %d needs distinct 4-byte aligned buffers and a row of a positive multiple of 4 bytes", j);
    c.src[k] = src[j];
    c.dst[k] = dst[j];
    c.words[k] = row_bytes[j] / 4;
  }
  hipLaunchKernelGGL(rnnt_greedy_commit_kernel, dim3(B, n_items), dim3(256), 0, (hipStream_t)stream, emit, c);
  return otr_check_launch("rnnt_greedy_commit");
}
