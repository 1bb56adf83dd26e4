// CTC loss (alpha/beta recursion) with the gradient taken straight to the logits, i.e. fused with the
// log_softmax backward.  Replaces nn.CTCLoss(blank=0, zero_infinity=True) (third-party torch kernel)
// as used by model/ctc.py:30,50-53; default reduction 'mean' = mean_b( nll_b / max(tgt_len_b, 1) ).
//
// One workgroup per utterance, one thread per extended-label state s (S = 2L+1 <= 256); the
// previous time step lives in a double-buffered LDS row, alpha is kept in a caller workspace for
// the beta pass.  d loss / d logit[b,t,c] = coef_b * ( softmax[b,t,c] - sum_{s: ext_s=c} gamma_t(s) ),
// gamma_t(s) = exp(alpha_t(s) + beta_t(s) - lp[t,ext_s] + nll_b),  coef_b = 1 / (B * max(L_b,1)).
#include "common.h"

#define NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ float lse3(float a, float b, float c) {
  float m = fmaxf(a, fmaxf(b, c));
  if (m == NEG_INF) return NEG_INF;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// dense part: dlogits = coef_b * exp(lp) for t < in_len[b], else 0; also zeroes *loss
__global__ void ctc_dense_kernel(const float* lp, float* dlogits, const int32_t* in_len, const int32_t* tgt_len,
                                 int B, int T, int V, float* loss) {
  const int64_t total = (int64_t)B * T * V;
  if (blockIdx.x == 0 && threadIdx.x == 0) *loss = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t bt = i / V;
    int b = (int)(bt / T), t = (int)(bt - (int64_t)b * T);
    float coef = 1.f / ((float)B * (float)max(tgt_len[b], 1));
    dlogits[i] = (t < in_len[b]) ? coef * expf(lp[i]) : 0.f;
  }
}

// The two recursions of one utterance by one workgroup, thread s on extended-label state s; otr_ctc_loss and otr_ctc_loss_pair share them.
// alpha: fills the utterance's table aw [Tb, Smax] and leaves its last two rows in sh (a barrier behind the last write).  `start`: the
// first frame opens states 0 and 1; without it every entry is -inf (no frames, or an utterance that must come out infeasible).
__device__ __forceinline__ void ctc_alpha_sweep(const float* lpb, float* aw, float (*sh)[256], int s, bool live, int S, int Tb, int V,
                                                int Smax, int blank, int ext, bool skip_b, bool start) {
  float a = NEG_INF;
  if (start) {
    if (s == 0) a = lpb[blank];
    else if (s == 1 && S > 1) a = lpb[ext];
  }
  sh[0][s] = a;
  if (live && Tb > 0) aw[s] = a;
  for (int t = 1; t < Tb; ++t) {
    __syncthreads();
    const float* prev = sh[(t - 1) & 1];
    float a0 = prev[s];
    float a1 = s >= 1 ? prev[s - 1] : NEG_INF;
    float a2 = skip_b ? prev[s - 2] : NEG_INF;
    a = live ? lse3(a0, a1, a2) + lpb[(int64_t)t * V + ext] : NEG_INF;
    sh[t & 1][s] = a;
    if (live) aw[(int64_t)t * Smax + s] = a;
  }
  __syncthreads();
}

// beta + occupancy: adds -wc * gamma_t(s) onto the utterance's gradient slab dl [T, V]; ll is finite (an alignment exists, Tb >= 1)
__device__ __forceinline__ void ctc_beta_sweep(const float* lpb, const float* aw, float* dl, float (*sh)[256], int s, bool live, int S,
                                               int Tb, int V, int Smax, int ext, bool skip_f, float ll, float wc) {
  float be = NEG_INF;
  {
    int t = Tb - 1;
    if (live && (s == S - 1 || s == S - 2)) be = lpb[(int64_t)t * V + ext];
    __syncthreads();
    sh[t & 1][s] = be;
    if (live && be != NEG_INF) {
      float g = expf(aw[(int64_t)t * Smax + s] + be - lpb[(int64_t)t * V + ext] - ll);
      atomicAdd(dl + (int64_t)t * V + ext, -wc * g);
    }
  }
  for (int t = Tb - 2; t >= 0; --t) {
    __syncthreads();
    const float* nxt = sh[(t + 1) & 1];
    float b0 = nxt[s];
    float b1 = (s + 1 < S) ? nxt[s + 1] : NEG_INF;
    float b2 = skip_f ? nxt[s + 2] : NEG_INF;
    float lpe = live ? lpb[(int64_t)t * V + ext] : 0.f;
    be = live ? lse3(b0, b1, b2) + lpe : NEG_INF;
    sh[t & 1][s] = be;
    if (live && be != NEG_INF) {
      float al = aw[(int64_t)t * Smax + s];
      if (al != NEG_INF) atomicAdd(dl + (int64_t)t * V + ext, -wc * expf(al + be - lpe - ll));
    }
  }
}

__global__ __launch_bounds__(256) void ctc_alpha_beta_kernel(const float* lp, const int64_t* targets, int64_t ldt,
                                                            const int32_t* in_len, const int32_t* tgt_len, int B, int T,
                                                            int V, int blank, float* alpha_ws, int Smax, float* nll_out,
                                                            float* loss, float* dlogits) {
  __shared__ float sh[2][256];
  __shared__ float s_ll;
  const int b = blockIdx.x, s = threadIdx.x;
  // a target length beyond the caller's bound (Smax = 2*max_tgt + 1 alpha slots per frame, `targets` rows of at least
  // max_tgt labels) would read `targets` out of bounds and write alpha rows over neighbouring (t, b) slots: such an
  // utterance is treated like an infeasible alignment (nll 0, zero gradient: zero_infinity semantics), never computed
  const int Lraw = tgt_len[b];
  const bool bad_len = Lraw < 0 || 2 * Lraw + 1 > Smax;
  const int Tb = max(min(in_len[b], T), 0), L = bad_len ? 0 : Lraw, S = 2 * L + 1;
  const float* lpb = lp + (int64_t)b * T * V;
  float* aw = alpha_ws + (int64_t)b * T * Smax;
  const int64_t* tg = targets + (int64_t)b * ldt;
  const bool live = s < S;
  const int ext = (live && (s & 1)) ? (int)tg[s >> 1] : blank;
  const int ext_m2 = (live && s >= 2 && (s & 1)) ? (int)tg[(s - 2) >> 1] : blank;
  const int ext_p2 = (s + 2 < S && (s & 1)) ? (int)tg[(s + 2) >> 1] : blank;
  const bool skip_b = live && s >= 2 && ext != blank && ext != ext_m2;       // s-2 -> s allowed
  const bool skip_f = (s + 2 < S) && ext_p2 != blank && ext_p2 != ext;       // s -> s+2 allowed
  const float coef = 1.f / ((float)B * (float)max(L, 1));

  ctc_alpha_sweep(lpb, aw, sh, s, live, S, Tb, V, Smax, blank, ext, skip_b, Tb > 0);
  if (s == 0) {
    float ll = NEG_INF;
    if (Tb > 0) {
      const float* fin = sh[(Tb - 1) & 1];
      ll = lse3(fin[S - 1], S > 1 ? fin[S - 2] : NEG_INF, NEG_INF);
    }
    if (bad_len) ll = NEG_INF;
    s_ll = ll;
    bool ok = ll != NEG_INF;                      // zero_infinity=True
    nll_out[b] = ok ? -ll : 0.f;
    if (ok) atomicAdd(loss, -ll * coef);
  }
  __syncthreads();
  const float ll = s_ll;
  if (!dlogits) return;
  if (ll == NEG_INF) {                            // infeasible alignment: zero the whole gradient slab
    for (int64_t i = s; i < (int64_t)T * V; i += 256) dlogits[(int64_t)b * T * V + i] = 0.f;
    return;
  }
  ctc_beta_sweep(lpb, aw, dlogits + (int64_t)b * T * V, sh, s, live, S, Tb, V, Smax, ext, skip_f, ll, coef);
}

extern "C" int32_t otr_ctc_loss(const float* log_probs, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                                const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank,
                                float* alpha_ws, float* nll, float* loss, float* dlogits, void* stream) {
  OTR_REQUIRE(log_probs && targets && in_len && tgt_len && alpha_ws && nll && loss, "ctc_loss: null pointer");
  OTR_REQUIRE(B > 0 && T > 0 && V > 1, "ctc_loss: bad shape B=%d T=%d V=%d", B, T, V);
  OTR_REQUIRE(max_tgt >= 0 && 2 * max_tgt + 1 <= 256, "ctc_loss: target length %d > 127 not supported", max_tgt);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_loss: blank out of range");
  hipStream_t s = (hipStream_t)stream;
  if (dlogits) {
    int64_t total = (int64_t)B * T * V;
    unsigned g = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(ctc_dense_kernel, dim3(g), dim3(256), 0, s, log_probs, dlogits, in_len, tgt_len, B, T, V, loss);
  } else {
    otr_zero_f32(loss, 1, s);
  }
  hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3(B), dim3(256), 0, s, log_probs, targets, ldt, in_len, tgt_len, B, T, V,
                     blank, alpha_ws, 2 * max_tgt + 1, nll, loss, dlogits);
  return otr_check_launch("ctc_loss");
}

// ------------------------------------------------------------------------------------------------ the paired form (MixSpeech)
// otr_ctc_loss_pair: ONE [P, T, V] table of log-probabilities scored against two label sets, k = 0 (a, weight lam) and k = 1 (b, weight
// 1 - lam), with one gradient lam * g_a + (1 - lam) * g_b.  Three launches:
//   1. ctc_pair_alpha_kernel, grid (P, 2): the alpha sweep of otr_ctc_loss for (utterance, set) into that set's alpha table, and nll.
//   2. ctc_pair_dense_kernel, grid (chunks, P): every cell of dlogits is written once, c_p * exp(lp) on the frames below in_len and zero
//      behind them, c_p = lam * ok_a * coef_a + (1 - lam) * ok_b * coef_b.  Whether a set has an alignment is known only now, after
//      both alpha sweeps (otr_ctc_loss writes the dense term first and zeroes the slab afterwards, which here would wipe the other
//      set's share).  Workgroup (0, 0) also adds up the three losses, in utterance order: no atomics, the same bits on every run.
//   3. ctc_pair_beta_kernel, grid (P, 2): the beta sweep; its occupancies, times the set's weight, are added onto the slab.  A set
//      without an alignment, or with weight exactly zero, returns before it touches anything.
// The log-likelihood of (utterance, set) is re-formed from the last alpha row wherever it is needed: the same three numbers through the
// same lse3 give the same bits, so no flag travels between the launches and the workspace is the two alpha tables.

// what the recursions of one (utterance, set) need; the guards are those of ctc_alpha_beta_kernel
struct CtcSeq {
  int Tb, L, S;
  bool bad_len;
  float coef;
};

__device__ __forceinline__ CtcSeq ctc_seq(const int32_t* in_len, const int32_t* tgt_len, int b, int B, int T, int Smax) {
  CtcSeq q;
  const int Lraw = tgt_len[b];
  q.bad_len = Lraw < 0 || 2 * Lraw + 1 > Smax;
  q.Tb = max(min(in_len[b], T), 0);
  q.L = q.bad_len ? 0 : Lraw;
  q.S = 2 * q.L + 1;
  q.coef = 1.f / ((float)B * (float)max(q.L, 1));
  return q;
}

// log-likelihood from the finished alpha table aw [T, Smax] of one (utterance, set); -inf: no alignment (zero_infinity) or guarded
__device__ __forceinline__ float ctc_ll_of(const float* aw, const CtcSeq& q, int Smax) {
  if (q.bad_len || q.Tb <= 0) return NEG_INF;
  const float* fin = aw + (int64_t)(q.Tb - 1) * Smax;
  return lse3(fin[q.S - 1], q.S > 1 ? fin[q.S - 2] : NEG_INF, NEG_INF);
}

__global__ __launch_bounds__(256) void ctc_pair_alpha_kernel(const float* lp, const int64_t* targets_a, int64_t ldt_a,
                                                            const int64_t* targets_b, int64_t ldt_b, const int32_t* in_len,
                                                            const int32_t* tgt_len_a, const int32_t* tgt_len_b, int B, int T, int V,
                                                            int blank, float* alpha_ws, int Smax, float* nll_out) {
  __shared__ float sh[2][256];
  const int b = blockIdx.x, k = blockIdx.y, s = threadIdx.x;
  const CtcSeq q = ctc_seq(in_len, k ? tgt_len_b : tgt_len_a, b, B, T, Smax);
  const int Tb = q.Tb, S = q.S;
  const float* lpb = lp + (int64_t)b * T * V;
  float* aw = alpha_ws + ((int64_t)k * B + b) * T * Smax;
  const int64_t* tg = k ? targets_b + (int64_t)b * ldt_b : targets_a + (int64_t)b * ldt_a;
  const bool live = s < S;
  const int64_t lab = (live && (s & 1)) ? tg[s >> 1] : (int64_t)blank;
  // a label outside [0, V) would index lp out of bounds: the whole (utterance, set) gets an alpha table of -inf, which every later
  // launch reads as "no alignment"
  const bool bad_label = __syncthreads_or(lab < 0 || lab >= V);
  const int ext = bad_label ? blank : (int)lab;
  const int ext_m2 = (live && s >= 2 && (s & 1) && !bad_label) ? (int)tg[(s - 2) >> 1] : blank;
  const bool skip_b = live && s >= 2 && ext != blank && ext != ext_m2;       // s-2 -> s allowed
  ctc_alpha_sweep(lpb, aw, sh, s, live, S, Tb, V, Smax, blank, ext, skip_b, Tb > 0 && !bad_label);
  if (s == 0) {
    float ll = NEG_INF;
    if (Tb > 0 && !q.bad_len) {
      const float* fin = sh[(Tb - 1) & 1];
      ll = lse3(fin[S - 1], S > 1 ? fin[S - 2] : NEG_INF, NEG_INF);
    }
    nll_out[(int64_t)k * B + b] = ll != NEG_INF ? -ll : 0.f;                 // zero_infinity=True
  }
}

constexpr int CTC_PAIR_CHUNK = 4096;                          // elements of a slab per workgroup of the dense kernel: 256 threads x 4 quads

__global__ __launch_bounds__(256) void ctc_pair_dense_kernel(const float* lp, const int32_t* in_len, const int32_t* tgt_len_a,
                                                            const int32_t* tgt_len_b, const float* lam_p, int B, int T, int V,
                                                            const float* alpha_ws, int Smax, const float* nll, float* loss3,
                                                            float* dlogits) {
  __shared__ float s_c;
  const int b = blockIdx.y, tid = threadIdx.x;
  const float lam = *lam_p;
  const float om = 1.f - lam;
  if (blockIdx.x == 0 && b == 0 && tid < 64) {                // the losses: lane i adds utterances i, i + 64, ... in order, then a butterfly
    float sa = 0.f, sb = 0.f;
    for (int u = tid; u < B; u += 64) {
      const CtcSeq qa = ctc_seq(in_len, tgt_len_a, u, B, T, Smax), qb = ctc_seq(in_len, tgt_len_b, u, B, T, Smax);
      sa += nll[u] * qa.coef;                                 // nll is 0 where there is no alignment
      sb += nll[(int64_t)B + u] * qb.coef;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sa += __shfl_xor(sa, o); sb += __shfl_xor(sb, o); }
    if (tid == 0) {
      loss3[0] = lam * sa + om * sb;
      loss3[1] = sa;
      loss3[2] = sb;
    }
  }
  if (!dlogits) return;
  const CtcSeq qa = ctc_seq(in_len, tgt_len_a, b, B, T, Smax);
  if (tid == 0) {
    const CtcSeq qb = ctc_seq(in_len, tgt_len_b, b, B, T, Smax);
    const bool ok_a = ctc_ll_of(alpha_ws + (int64_t)b * T * Smax, qa, Smax) != NEG_INF;
    const bool ok_b = ctc_ll_of(alpha_ws + ((int64_t)B + b) * T * Smax, qb, Smax) != NEG_INF;
    s_c = (ok_a ? lam * qa.coef : 0.f) + (ok_b ? om * qb.coef : 0.f);
  }
  __syncthreads();
  const float c = s_c;
  const int64_t TV = (int64_t)T * V, n = c != 0.f ? (int64_t)qa.Tb * V : 0;       // Tb is in_len clamped: the same for both sets
  const float* x = lp + (int64_t)b * TV;
  float* y = dlogits + (int64_t)b * TV;
  const bool xvec = ((uintptr_t)x & 15) == 0, yvec = ((uintptr_t)y & 15) == 0;
  const int64_t e0 = (int64_t)blockIdx.x * CTC_PAIR_CHUNK;
#pragma unroll
  for (int q = 0; q < CTC_PAIR_CHUNK / 1024; ++q) {
    const int64_t e = e0 + (int64_t)(q * 256 + tid) * 4;
    if (e >= TV) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < n) {
      if (xvec && e + 4 <= n) {
        const uint4 u = ld_global_b128(x + e);
        v[0] = c * expf(__uint_as_float(u.x)); v[1] = c * expf(__uint_as_float(u.y));
        v[2] = c * expf(__uint_as_float(u.z)); v[3] = c * expf(__uint_as_float(u.w));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < n) v[k] = c * expf(x[e + k]);
      }
    }
    if (yvec && e + 4 <= TV) {
      st_global_b128(y + e, make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < TV) y[e + k] = v[k];
    }
  }
}

__global__ __launch_bounds__(256) void ctc_pair_beta_kernel(const float* lp, const int64_t* targets_a, int64_t ldt_a,
                                                           const int64_t* targets_b, int64_t ldt_b, const int32_t* in_len,
                                                           const int32_t* tgt_len_a, const int32_t* tgt_len_b, const float* lam_p, int B,
                                                           int T, int V, int blank, const float* alpha_ws, int Smax, float* dlogits) {
  __shared__ float sh[2][256];
  const int b = blockIdx.x, k = blockIdx.y, s = threadIdx.x;
  const float lam = *lam_p;
  const float w = k ? 1.f - lam : lam;
  if (w == 0.f) return;                                       // a set of weight zero adds nothing, whatever its labels are
  const CtcSeq q = ctc_seq(in_len, k ? tgt_len_b : tgt_len_a, b, B, T, Smax);
  const float* aw = alpha_ws + ((int64_t)k * B + b) * T * Smax;
  const float ll = ctc_ll_of(aw, q, Smax);                    // workgroup-uniform
  if (ll == NEG_INF) return;                                  // no alignment: the other set's share of the slab stays as it is
  const int Tb = q.Tb, S = q.S;
  const float* lpb = lp + (int64_t)b * T * V;
  const int64_t* tg = k ? targets_b + (int64_t)b * ldt_b : targets_a + (int64_t)b * ldt_a;
  const bool live = s < S;
  const int ext = (live && (s & 1)) ? (int)tg[s >> 1] : blank;
  const int ext_p2 = (s + 2 < S && (s & 1)) ? (int)tg[(s + 2) >> 1] : blank;
  const bool skip_f = (s + 2 < S) && ext_p2 != blank && ext_p2 != ext;       // s -> s+2 allowed
  ctc_beta_sweep(lpb, aw, dlogits + (int64_t)b * T * V, sh, s, live, S, Tb, V, Smax, ext, skip_f, ll, w * q.coef);
}

extern "C" int32_t otr_ctc_loss_pair(const float* log_probs, const int64_t* targets_a, int64_t ldt_a, const int32_t* tgt_len_a,
                                     const int64_t* targets_b, int64_t ldt_b, const int32_t* tgt_len_b, const int32_t* in_len,
                                     const float* lam, int32_t P, int32_t T, int32_t V, int32_t max_tgt, int32_t blank, float* alpha_ws,
                                     float* nll, float* loss3, float* dlogits, void* stream) {
  OTR_REQUIRE(log_probs && targets_a && targets_b && tgt_len_a && tgt_len_b && in_len && lam && alpha_ws && nll && loss3,
              "ctc_loss_pair: null pointer");
  OTR_REQUIRE(P > 0 && P <= 65535 && T > 0 && V > 1, "ctc_loss_pair: bad shape P=%d T=%d V=%d", P, T, V);
  OTR_REQUIRE(max_tgt >= 0 && 2 * max_tgt + 1 <= 256, "ctc_loss_pair: target length %d > 127 not supported", max_tgt);
  OTR_REQUIRE(ldt_a >= max_tgt && ldt_b >= max_tgt, "ctc_loss_pair: target row strides %lld, %lld below max_tgt = %d", (long long)ldt_a,
              (long long)ldt_b, max_tgt);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_loss_pair: blank out of range");
  hipStream_t s = (hipStream_t)stream;
  const int Smax = 2 * max_tgt + 1;
  hipLaunchKernelGGL(ctc_pair_alpha_kernel, dim3(P, 2), dim3(256), 0, s, log_probs, targets_a, ldt_a, targets_b, ldt_b, in_len, tgt_len_a,
                     tgt_len_b, P, T, V, blank, alpha_ws, Smax, nll);
  const int64_t TV = (int64_t)T * V;
  const unsigned nchunk = dlogits ? (unsigned)((TV + CTC_PAIR_CHUNK - 1) / CTC_PAIR_CHUNK) : 1u;
  hipLaunchKernelGGL(ctc_pair_dense_kernel, dim3(nchunk, dlogits ? P : 1), dim3(256), 0, s, log_probs, in_len, tgt_len_a, tgt_len_b, lam, P,
                     T, V, (const float*)alpha_ws, Smax, (const float*)nll, loss3, dlogits);
  if (dlogits)
    hipLaunchKernelGGL(ctc_pair_beta_kernel, dim3(P, 2), dim3(256), 0, s, log_probs, targets_a, ldt_a, targets_b, ldt_b, in_len, tgt_len_a,
                       tgt_len_b, lam, P, T, V, blank, (const float*)alpha_ws, Smax, dlogits);
  return otr_check_launch("ctc_loss_pair");
}

// ------------------------------------------------------------------------------------------------ the N-best form (MWER for the CTC model)
// otr_ctc_mwer_loss: ONE [B, T, V] table of log-probabilities scored against N hypotheses per utterance and, optionally, the reference:
// the pair form with N + 1 label sets and a posterior step between the sweeps (include/otrans_hip.h states the semantics).  Four launches:
//   1. ctc_mwer_alpha_kernel, grid (B, N or N + 1): the alpha sweep of (utterance, slot) into that slot's alpha table; slot N is the
//      reference.  It leaves ll in seq_logp (-inf: the slot is dead) and the reference's nll in nll_ref.
//   2. ctc_mwer_post_kernel, ONE workgroup over the B x N scalars, as mwer_post_kernel: P, E_b, the three losses through one LDS tree
//      (the same bits on every run) and the weight wc of every (utterance, slot) the beta sweep multiplies its occupancies by.
//   3. ctc_mwer_dense_kernel, grid (chunks, B): every cell of dlogits is written once.  sum_n c_n = 0 cancels the softmax term of the
//      hypotheses, so only the reference's survives: wc_ref * exp(lp) on the frames below in_len, and zeros -- lp is not read -- behind
//      them and wherever wc_ref is 0 (no reference, ctc_weight 0, no alignment).
//   4. ctc_mwer_beta_kernel, grid (B, N or N + 1): the beta sweep adds -wc * gamma onto the slab; a weight of exactly 0 returns first.
// As in the pair form the log-likelihood is re-formed from the last alpha row where it is needed; the workspace is the N + 1 alpha
// tables and the B x (N + 1) weights.

// the sequence of (utterance b, slot k): k < N hypothesis k, k == N the reference
__device__ __forceinline__ CtcSeq ctc_mwer_seq(const int32_t* in_len, const int32_t* hyp_len, const int32_t* ref_len, int b, int k, int B,
                                               int N, int T, int Smax) {
  return k < N ? ctc_seq(in_len + b, hyp_len + (int64_t)b * N + k, 0, B, T, Smax) : ctc_seq(in_len, ref_len, b, B, T, Smax);
}

__global__ __launch_bounds__(256) void ctc_mwer_alpha_kernel(const float* lp, const int32_t* in_len, const int64_t* hyps, int64_t ldh,
                                                            const int32_t* hyp_len, const int32_t* errors, const int64_t* ref, int64_t ldr,
                                                            const int32_t* ref_len, int B, int N, int T, int V, int blank, float* alpha_ws,
                                                            int Smax, float* seq_logp, float* nll_ref) {
  __shared__ float sh[2][256];
  const int b = blockIdx.x, k = blockIdx.y, s = threadIdx.x;
  const int64_t h = (int64_t)b * N + k;
  if (k < N && errors[h] < 0) {                               // an invalid pair: nothing of the slot is read
    if (s == 0) seq_logp[h] = NEG_INF;
    return;
  }
  const CtcSeq q = ctc_mwer_seq(in_len, hyp_len, ref_len, b, k, B, N, T, Smax);
  const int Tb = q.Tb, S = q.S;
  const float* lpb = lp + (int64_t)b * T * V;
  float* aw = alpha_ws + ((int64_t)k * B + b) * T * Smax;
  const int64_t* tg = k < N ? hyps + h * ldh : ref + (int64_t)b * ldr;
  const bool live = s < S;
  const int64_t lab = (live && (s & 1)) ? tg[s >> 1] : (int64_t)blank;
  // a label outside [0, V): an alpha table of -inf, which every later launch reads as "no alignment" (ctc_pair_alpha_kernel)
  const bool bad_label = __syncthreads_or(lab < 0 || lab >= V);
  const int ext = bad_label ? blank : (int)lab;
  const int ext_m2 = (live && s >= 2 && (s & 1) && !bad_label) ? (int)tg[(s - 2) >> 1] : blank;
  const bool skip_b = live && s >= 2 && ext != blank && ext != ext_m2;       // s-2 -> s allowed
  ctc_alpha_sweep(lpb, aw, sh, s, live, S, Tb, V, Smax, blank, ext, skip_b, Tb > 0 && !bad_label);
  if (s == 0) {
    float ll = NEG_INF;
    if (Tb > 0 && !q.bad_len) {
      const float* fin = sh[(Tb - 1) & 1];
      ll = lse3(fin[S - 1], S > 1 ? fin[S - 2] : NEG_INF, NEG_INF);
    }
    if (k < N) seq_logp[h] = ll;
    else nll_ref[b] = ll != NEG_INF ? -ll : 0.f;               // zero_infinity=True
  }
}

__global__ __launch_bounds__(256) void ctc_mwer_post_kernel(const float* seq_logp, const int32_t* errors, const int32_t* in_len,
                                                           const int32_t* ref_len, int B, int N, int T, int Smax, float ctc_weight,
                                                           float scale, const float* gscale, const float* alpha_ws, float* nll_ref,
                                                           float* loss3, float* post, float* utt_err, float* wc) {
  __shared__ float s_sum[256], s_ctc[256];
  __shared__ int s_cnt[256];
  const int tid = threadIdx.x;
  const float g = gscale ? *gscale : 1.f;
  float esum = 0.f, csum = 0.f;
  int cnt = 0;
  for (int b = tid; b < B; b += 256) {
    const float* s = seq_logp + (int64_t)b * N;
    const int32_t* w = errors + (int64_t)b * N;
    float* p = post + (int64_t)b * N;
    float m = NEG_INF;
    bool any = false;
    for (int n = 0; n < N; ++n)
      if (!(s[n] == NEG_INF)) {
        m = fmaxf(m, scale * s[n]);
        any = true;
      }
    float z = 0.f;
    for (int n = 0; n < N; ++n)
      if (!(s[n] == NEG_INF)) z += expf(scale * s[n] - m);
    float e = 0.f;
    for (int n = 0; n < N; ++n) {
      const float pn = !(s[n] == NEG_INF) ? expf(scale * s[n] - m) / z : 0.f;
      p[n] = pn;
      if (pn != 0.f) e += pn * (float)w[n];
    }
    utt_err[b] = e;
    if (any) {
      esum += e;
      ++cnt;
    }
    // the reference: its nll times coef, and the weight of its dense term and of its occupancies
    float wr = 0.f;
    if (ref_len) {
      const CtcSeq q = ctc_seq(in_len, ref_len, b, B, T, Smax);
      if (ctc_ll_of(alpha_ws + ((int64_t)N * B + b) * T * Smax, q, Smax) != NEG_INF) {
        csum += nll_ref[b] * q.coef;
        wr = g * ctc_weight * q.coef;
      }
    } else {
      nll_ref[b] = 0.f;
    }
    wc[(int64_t)b * (N + 1) + N] = wr;
  }
  s_sum[tid] = esum;
  s_ctc[tid] = csum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                 // one tree, the same order on every run
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_ctc[tid] += s_ctc[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
    }
    __syncthreads();
  }
  const int b_live = s_cnt[0];
  if (tid == 0) {
    const float mwer = b_live > 0 ? s_sum[0] / (float)b_live : 0.f;
    loss3[0] = mwer + ctc_weight * s_ctc[0];
    loss3[1] = mwer;
    loss3[2] = s_ctc[0];
  }
  for (int b = tid; b < B; b += 256) {                // this thread wrote post and utt_err of these utterances
    const float e = utt_err[b];
    for (int n = 0; n < N; ++n) {
      const int64_t h = (int64_t)b * N + n;
      const float pn = post[h];                       // wc = -g c_n / B_live: the beta sweep adds -wc * gamma
      wc[(int64_t)b * (N + 1) + n] = pn != 0.f ? -(g * (scale * pn * ((float)errors[h] - e)) / (float)b_live) : 0.f;
    }
  }
}

// the chunk body is ctc_pair_dense_kernel's, repeated: sharing it as one inline function gives that kernel another register allocation,
// and the device code of otr_ctc_loss_pair stays what it was
__global__ __launch_bounds__(256) void ctc_mwer_dense_kernel(const float* lp, const int32_t* in_len, int N, int T, int V, const float* wc,
                                                            float* dlogits) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const float c = wc[(int64_t)b * (N + 1) + N];
  const int Tb = max(min(in_len[b], T), 0);
  const int64_t TV = (int64_t)T * V, n = c != 0.f ? (int64_t)Tb * V : 0;
  const float* x = lp + (int64_t)b * TV;
  float* y = dlogits + (int64_t)b * TV;
  const bool xvec = ((uintptr_t)x & 15) == 0, yvec = ((uintptr_t)y & 15) == 0;
  const int64_t e0 = (int64_t)blockIdx.x * CTC_PAIR_CHUNK;
#pragma unroll
  for (int q = 0; q < CTC_PAIR_CHUNK / 1024; ++q) {
    const int64_t e = e0 + (int64_t)(q * 256 + tid) * 4;
    if (e >= TV) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < n) {
      if (xvec && e + 4 <= n) {
        const uint4 u = ld_global_b128(x + e);
        v[0] = c * expf(__uint_as_float(u.x)); v[1] = c * expf(__uint_as_float(u.y));
        v[2] = c * expf(__uint_as_float(u.z)); v[3] = c * expf(__uint_as_float(u.w));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < n) v[k] = c * expf(x[e + k]);
      }
    }
    if (yvec && e + 4 <= TV) {
      st_global_b128(y + e, make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < TV) y[e + k] = v[k];
    }
  }
}

__global__ __launch_bounds__(256) void ctc_mwer_beta_kernel(const float* lp, const int32_t* in_len, const int64_t* hyps, int64_t ldh,
                                                           const int32_t* hyp_len, const int64_t* ref, int64_t ldr, const int32_t* ref_len,
                                                           int B, int N, int T, int V, int blank, const float* alpha_ws, int Smax,
                                                           const float* wc, float* dlogits) {
  __shared__ float sh[2][256];
  const int b = blockIdx.x, k = blockIdx.y, s = threadIdx.x;
  const float w = wc[(int64_t)b * (N + 1) + k];
  if (w == 0.f) return;                                       // a dead slot, P_n (W_n - E_b) == 0 (every slot at N = 1), or no CTC term
  const CtcSeq q = ctc_mwer_seq(in_len, hyp_len, ref_len, b, k, B, N, T, Smax);
  const float* aw = alpha_ws + ((int64_t)k * B + b) * T * Smax;
  const float ll = ctc_ll_of(aw, q, Smax);                    // workgroup-uniform; finite: the post step gives a weight to live slots only
  if (ll == NEG_INF) return;
  const int Tb = q.Tb, S = q.S;
  const float* lpb = lp + (int64_t)b * T * V;
  const int64_t* tg = k < N ? hyps + ((int64_t)b * N + k) * ldh : ref + (int64_t)b * ldr;
  const bool live = s < S;
  const int ext = (live && (s & 1)) ? (int)tg[s >> 1] : blank;
  const int ext_p2 = (s + 2 < S && (s & 1)) ? (int)tg[(s + 2) >> 1] : blank;
  const bool skip_f = (s + 2 < S) && ext_p2 != blank && ext_p2 != ext;       // s -> s+2 allowed
  ctc_beta_sweep(lpb, aw, dlogits + (int64_t)b * T * V, sh, s, live, S, Tb, V, Smax, ext, skip_f, ll, w);
}

static bool ctc_mwer_shape_ok(int64_t B, int64_t N, int64_t T, int64_t max_tgt) {
  return B >= 1 && B <= 65535 && N >= 1 && N <= 32 && T >= 1 && max_tgt >= 0 && max_tgt <= 127;
}

extern "C" int64_t otr_ctc_mwer_workspace_floats(int32_t B, int32_t N, int32_t T, int32_t max_tgt) {
  if (!ctc_mwer_shape_ok(B, N, T, max_tgt)) return -1;
  return ((int64_t)N + 1) * B * T * (2 * max_tgt + 1) + (int64_t)B * (N + 1);     // the N + 1 alpha tables, then the weights
}

extern "C" int32_t otr_ctc_mwer_loss(const float* log_probs, const int32_t* in_len, const int64_t* hyps, int64_t ldh, const int32_t* hyp_len,
                                     const int32_t* errors, const int64_t* ref, int64_t ldr, const int32_t* ref_len, float ctc_weight,
                                     float scale, const float* gscale, int32_t B, int32_t N, int32_t T, int32_t V, int32_t max_tgt,
                                     int32_t blank, float* loss3, float* seq_logp, float* post, float* utt_err, float* nll_ref,
                                     float* dlogits, float* workspace, int64_t workspace_floats, void* stream) {
  OTR_REQUIRE(log_probs && in_len && hyps && hyp_len && errors && loss3 && seq_logp && post && utt_err && nll_ref && workspace,
              "ctc_mwer_loss: null pointer");
  OTR_REQUIRE((ref != nullptr) == (ref_len != nullptr) && (ref || ldr == 0), "ctc_mwer_loss: ref, ldr and ref_len go together (all or none)");
  OTR_REQUIRE(ctc_mwer_shape_ok(B, N, T, max_tgt) && V >= 2,
              "ctc_mwer_loss: bad shape B=%d N=%d T=%d V=%d max_tgt=%d (B 1 .. 65535, N 1 .. 32, max_tgt 0 .. 127)", B, N, T, V, max_tgt);
  OTR_REQUIRE(ldh >= max_tgt && (!ref || ldr >= max_tgt), "ctc_mwer_loss: label row strides %lld, %lld below max_tgt = %d", (long long)ldh,
              (long long)ldr, max_tgt);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_mwer_loss: blank out of range");
  OTR_REQUIRE(ctc_weight >= 0.f && ctc_weight < __builtin_huge_valf() && scale > 0.f && scale < __builtin_huge_valf(),
              "ctc_mwer_loss: ctc_weight=%g must be finite and >= 0, scale=%g finite and > 0", (double)ctc_weight, (double)scale);
  const int64_t need = otr_ctc_mwer_workspace_floats(B, N, T, max_tgt);
  OTR_REQUIRE(need >= 0 && workspace_floats >= need, "ctc_mwer_loss: workspace of %lld floats, %lld needed", (long long)workspace_floats,
              (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const int Smax = 2 * max_tgt + 1, K = N + (ref ? 1 : 0);
  float* wc = workspace + ((int64_t)N + 1) * B * T * Smax;
  hipLaunchKernelGGL(ctc_mwer_alpha_kernel, dim3(B, K), dim3(256), 0, s, log_probs, in_len, hyps, ldh, hyp_len, errors, ref, ldr, ref_len, B, N,
                     T, V, blank, workspace, Smax, seq_logp, nll_ref);
  hipLaunchKernelGGL(ctc_mwer_post_kernel, dim3(1), dim3(256), 0, s, (const float*)seq_logp, errors, in_len, ref_len, B, N, T, Smax, ctc_weight,
                     scale, gscale, (const float*)workspace, nll_ref, loss3, post, utt_err, wc);
  if (dlogits) {
    const int64_t TV = (int64_t)T * V;
    hipLaunchKernelGGL(ctc_mwer_dense_kernel, dim3((unsigned)((TV + CTC_PAIR_CHUNK - 1) / CTC_PAIR_CHUNK), B), dim3(256), 0, s, log_probs, in_len,
                       N, T, V, (const float*)wc, dlogits);
    hipLaunchKernelGGL(ctc_mwer_beta_kernel, dim3(B, K), dim3(256), 0, s, log_probs, in_len, hyps, ldh, hyp_len, ref, ldr, ref_len, B, N, T, V,
                       blank, (const float*)workspace, Smax, (const float*)wc, dlogits);
  }
  return otr_check_launch("ctc_mwer_loss");
}
