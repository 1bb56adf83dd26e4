// Joint CTC/attention beam search (SpeechToTextRecognizer joint_ctc=True; Watanabe et al. 2017, Algorithm 2): the CTC prefix score
// of every candidate extension, on the device, inside the (captured) decode step.  include/otrans_hip.h states the semantics.  f32 in
// both builds.
//  * joint_prebeam:    per hypothesis row: (1-lambda) * log_softmax(att) + lm_weight * log_softmax(lm) fused with the top-K' over the
//                      vocabulary (descending, ties -> lower token).  The row sits in registers; the K'-th largest score is found by a
//                      16-round (two bits each) search over block-wide counts of order-preserving u32 keys, the winners are compacted and
//                      ranked in LDS.  The log-softmax is formed exactly as otr_beam_topk forms it.
//  * ctc_prefix_score: per hypothesis row: the parent prefix's phi (from its (r^n, r^b)) and the blank column go to LDS, the K'
//                      candidates' columns are staged JS_TC frames at a time -- waves 1-3 load the next chunk while wave 0 runs the
//                      recurrence on this one, one lane per candidate -- then the joint score and the top-beam of the K'.
#include "common.h"

#define NEG_INF (-__builtin_huge_valf())

constexpr int JS_MAXK = 32;       // pre-beam K'
constexpr int JS_MAXBEAM = 16;    // the prune's limit
constexpr int JS_MAXT = 2048;     // frames T' (the parent's phi and the blank column live in LDS)
constexpr int JS_MAXV = 8192;     // vocabulary of the pre-beam (32 scores per thread)
constexpr int JS_TC = 128;        // frames per staged chunk

__device__ __forceinline__ uint32_t js_key(float x) {   // order-preserving: a > b <=> key(a) > key(b); -0 folded onto +0; 0 = no key
  const uint32_t u = __float_as_uint(x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int js_wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// a store that stays a global_store: a pointer picked at run time (or null) may compile to flat_store, which counts on lgkmcnt too, and
// every LDS read of the recurrence behind it would wait for the store to reach memory
__device__ __forceinline__ void js_st(float* p, float v) { *(OTR_GLOBAL float*)p = v; }
// log(exp a + exp b) on the hardware exp2 / log2, branch-free: where both are -inf, d = -inf (not NaN), the log term is 0 and the
// result m = -inf.  (An early return for m == -inf made each log-add-exp a branch of its own and serialised the recurrence's three
// chains: 70 us per step at T' 249.)
__device__ __forceinline__ float js_lae(float a, float b) {
  const float m = fmaxf(a, b);
  const float d = fminf(a, b) - fmaxf(m, -3.402823466e38f);
  return fmaf(__builtin_amdgcn_logf(1.f + __builtin_amdgcn_exp2f(d * 1.4426950408889634f)), 0.6931471805599453f, m);
}

// ---------------------------------------------------------------- pre-beam top-K'
template <int NV>
__global__ __launch_bounds__(256) void joint_prebeam_kernel(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm,
                                                            float att_w, float lm_w, int V, int K, float* out_s, int32_t* out_i) {
  __shared__ float shf[8];
  __shared__ int shi[2][4], sh3[2][4];
  __shared__ float c_s[JS_MAXK];
  __shared__ int c_i[JS_MAXK];
  __shared__ int nsel;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t row = blockIdx.x;
  const float* x = logits + row * ld;
  const float* y = lm_logits ? lm_logits + row * ld_lm : nullptr;
  float xs[NV], ys[NV];
  float mx = NEG_INF, my = NEG_INF;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = tid + 256 * j;
    xs[j] = v < V ? x[v] : NEG_INF;
    ys[j] = (y && v < V) ? y[v] : NEG_INF;
    mx = fmaxf(mx, xs[j]);
    my = fmaxf(my, ys[j]);
  }
  // the log-softmax of both rows exactly as otr_beam_topk forms it (same partial sums in the same order): at lambda = 0 the pre-beam
  // scores are bit-identical to the plain search's
  mx = wave_max(mx); my = wave_max(my);
  if (lane == 0) { shf[wid] = mx; shf[4 + wid] = my; }
  __syncthreads();
  mx = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
  my = fmaxf(fmaxf(shf[4], shf[5]), fmaxf(shf[6], shf[7]));
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = tid + 256 * j;
    if (v < V) { sx += expf(xs[j] - mx); if (y) sy += expf(ys[j] - my); }
  }
  sx = wave_sum(sx); sy = wave_sum(sy);
  __syncthreads();
  if (lane == 0) { shf[wid] = sx; shf[4 + wid] = sy; }
  __syncthreads();
  const float lse = mx + logf(shf[0] + shf[1] + shf[2] + shf[3]);
  const float llse = y ? my + logf(shf[4] + shf[5] + shf[6] + shf[7]) : 0.f;
  float sc[NV];
  uint32_t key[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = tid + 256 * j;
    float s = xs[j] - lse;
    if (att_w != 1.f) s *= att_w;
    if (y) s += lm_w * (ys[j] - llse);
    if (!(s == s)) s = NEG_INF;                       // NaN ranks as -inf, as in otr_beam_topk
    sc[j] = s;
    key[j] = v < V ? js_key(s) : 0u;
  }
  // tau = the K-th largest key (K <= V: at least K real keys, all > 0), two bits per round: the counts at three thresholds, two of them
  // packed in the halves of one int (a block holds <= 8192 keys)
  uint32_t tau = 0;
  for (int sh = 30; sh >= 0; sh -= 2) {
    const uint32_t c1 = tau | (1u << sh), c2 = tau | (2u << sh), c3 = tau | (3u << sh);
    int p12 = 0, p3 = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) { p12 += (int)(key[j] >= c1) + ((int)(key[j] >= c2) << 16); p3 += key[j] >= c3; }
    p12 = js_wave_isum(p12); p3 = js_wave_isum(p3);
    const int buf = (sh >> 1) & 1;                    // double-buffered: one barrier per round
    if (lane == 0) { shi[buf][wid] = p12; sh3[buf][wid] = p3; }
    __syncthreads();
    const int s12 = shi[buf][0] + shi[buf][1] + shi[buf][2] + shi[buf][3];
    const int s3 = sh3[buf][0] + sh3[buf][1] + sh3[buf][2] + sh3[buf][3];
    tau = s3 >= K ? c3 : (s12 >> 16) >= K ? c2 : (s12 & 0xffff) >= K ? c1 : tau;
  }
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) { gt += key[j] > tau; eq += key[j] == tau; }
  gt = js_wave_isum(gt); eq = js_wave_isum(eq);
  __syncthreads();
  if (lane == 0) { shi[0][wid] = gt; shi[1][wid] = eq; }
  if (tid == 0) nsel = 0;
  __syncthreads();
  gt = shi[0][0] + shi[0][1] + shi[0][2] + shi[0][3];
  eq = shi[1][0] + shi[1][1] + shi[1][2] + shi[1][3];
  const int need = K - gt;                            // >= 1 keys equal to tau are taken, lowest tokens first
  __syncthreads();
  if (eq == need) {                                   // (uniform) the usual case: every key >= tau
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (key[j] >= tau) { const int p = atomicAdd(&nsel, 1); c_s[p] = sc[j]; c_i[p] = tid + 256 * j; }
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (key[j] > tau) { const int p = atomicAdd(&nsel, 1); c_s[p] = sc[j]; c_i[p] = tid + 256 * j; }
    // ties at tau: in ascending token order, v = tid + 256 j (j-major, then the thread)
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    int seen = 0;
    for (int j = 0; j < NV; ++j) {
      const bool e = key[j] == tau;
      const uint64_t m = __ballot(e);
      if (lane == 0) shi[j & 1][wid] = __popcll(m);
      __syncthreads();
      int before = seen;
      for (int w = 0; w < wid; ++w) before += shi[j & 1][w];
      if (e && before + __popcll(m & lt_mask) < need) { const int p = atomicAdd(&nsel, 1); c_s[p] = sc[j]; c_i[p] = tid + 256 * j; }
      seen += shi[j & 1][0] + shi[j & 1][1] + shi[j & 1][2] + shi[j & 1][3];
    }
  }
  __syncthreads();
  if (tid < K) {
    const float s = c_s[tid];
    const int i = c_i[tid];
    int r = 0;
    for (int q = 0; q < K; ++q) r += c_s[q] > s || (c_s[q] == s && c_i[q] < i);
    out_s[row * K + r] = s;
    out_i[row * K + r] = i;
  }
}

extern "C" int32_t otr_joint_prebeam(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm, float att_weight,
                                     float lm_weight, int64_t rows, int32_t V, int32_t K, float* cand_score, int32_t* cand_idx,
                                     void* stream) {
  OTR_REQUIRE(logits && cand_score && cand_idx, "joint_prebeam: null pointer");
  OTR_REQUIRE(V >= 1 && V <= JS_MAXV && ld >= V && (!lm_logits || ld_lm >= V), "joint_prebeam: V=%d must be in [1, %d], ld >= V", V,
              JS_MAXV);
  OTR_REQUIRE(K >= 1 && K <= JS_MAXK && K <= V, "joint_prebeam: K=%d must be in [1, min(%d, V=%d)]", K, JS_MAXK, V);
  OTR_REQUIRE(rows >= 0 && rows < (1ll << 31), "joint_prebeam: bad rows");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)rows), b(256);
  if (V <= 256 * 8)
    hipLaunchKernelGGL(joint_prebeam_kernel<8>, g, b, 0, s, logits, ld, lm_logits, ld_lm, att_weight, lm_weight, V, K, cand_score, cand_idx);
  else if (V <= 256 * 20)
    hipLaunchKernelGGL(joint_prebeam_kernel<20>, g, b, 0, s, logits, ld, lm_logits, ld_lm, att_weight, lm_weight, V, K, cand_score, cand_idx);
  else
    hipLaunchKernelGGL(joint_prebeam_kernel<32>, g, b, 0, s, logits, ld, lm_logits, ld_lm, att_weight, lm_weight, V, K, cand_score, cand_idx);
  return otr_check_launch("joint_prebeam");
}

// ---------------------------------------------------------------- CTC prefix score + joint top-beam
__global__ __launch_bounds__(256) void ctc_prefix_score_kernel(
    const float* lp, int64_t ld, const int32_t* lengths, int T, int V, int blank, int eos, int rows_per_utt, int K,
    const int32_t* cand_idx, const float* cand_score, const uint8_t* flags, const int64_t* preds, int64_t ldp, int t_host,
    const int32_t* pos, const int32_t* jsrc, const float* rn_in, const float* rb_in, const float* psi_in, float ctc_w, float* rn_out,
    float* rb_out, float* psi_out, int beam, float* k_score, int64_t* k_idx, int32_t* k_src) {
  __shared__ float s_x[2][JS_MAXK][JS_TC + 1];       // candidate columns of a chunk of frames (+1: lanes k hit distinct banks)
  __shared__ float s_blank[JS_MAXT], s_phid[JS_MAXT], s_phis[JS_MAXT];
  __shared__ int s_c[JS_MAXK];
  __shared__ float s_psi[JS_MAXK], s_j[JS_MAXK];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t row = blockIdx.x;
  const int t = pos ? *pos + 1 : t_host;              // prefix columns: BOS + n tokens
  const int n = t - 1;
  if (flags && flags[row]) {                          // finished: the CTC head is not consulted (the prune masks this row's entries)
    if (k_score && tid < beam) {
      k_score[row * beam + tid] = NEG_INF;
      k_idx[row * beam + tid] = eos;
      k_src[row * beam + tid] = -1;
    }
    return;
  }
  const int b = (int)(row / rows_per_utt);
  const int Tb = min(max(lengths[b], 1), T);
  const float* x = lp + (int64_t)b * T * ld;
  const int last = n >= 1 ? (int)preds[row * ldp + n] : -1;
  if (tid < K) s_c[tid] = cand_idx[row * K + tid];
  for (int tt = tid; tt < Tb; tt += 256) s_blank[tt] = x[(int64_t)tt * ld + blank];
  float psi_g = 0.f;
  if (n >= 1) {
    const int64_t src = jsrc[row];
    psi_g = src >= 0 ? psi_in[src] : NEG_INF;
    for (int tt = tid; tt < Tb; tt += 256) {
      const float rn = src >= 0 ? rn_in[src * T + tt] : NEG_INF, rb = src >= 0 ? rb_in[src * T + tt] : NEG_INF;
      s_phis[tt] = rb;                                // phi for c == last(g)
      s_phid[tt] = js_lae(rn, rb);                    // phi for any other c
    }
  }
  __syncthreads();
  if (n == 0 && tid == 0) {                           // the start prefix: r^n = -inf, r^b_t = sum_{tau <= t} x_tau(blank)
    float a = 0.f;
    for (int tt = 0; tt < Tb; ++tt) { a += s_blank[tt]; s_phis[tt] = a; s_phid[tt] = a; }
  }
  // a chunk's K' x JS_TC elements, every load of a thread issued before the first LDS store (one memory latency per chunk, not one
  // per element: a rolled loop waited for each scattered load in turn)
  auto stage = [&](int ci, int first, int stride) {
    constexpr int NL = (JS_MAXK * JS_TC + 191) / 192;
    const int t0 = ci * JS_TC;
    float v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = first + i * stride, tt = e / K, k = e - tt * K;   // consecutive threads: the candidates of one frame (one row of lp)
      const int c = e < K * JS_TC ? s_c[k] : -1;
      v[i] = (e < K * JS_TC && t0 + tt < Tb && c >= 0 && c < V) ? x[(int64_t)(t0 + tt) * ld + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = first + i * stride, tt = e / K, k = e - tt * K;
      if (e < K * JS_TC) s_x[ci & 1][k][tt] = v[i];
    }
  };
  stage(0, tid, 256);
  __syncthreads();
  const int nchunk = (Tb + JS_TC - 1) / JS_TC;
  int c = -1;
  bool live = false;
  const float* phi = s_phid;
  float rn = NEG_INF, rb = NEG_INF, psi = NEG_INF;
  float *rno = nullptr, *rbo = nullptr;
  if (wid == 0 && lane < K) {
    c = s_c[lane];
    live = c != blank && c != eos && c >= 0 && c < V;
    phi = c == last ? s_phis : s_phid;
    if (c == eos) psi = s_phid[Tb - 1];               // log(r^n_{T_b-1}(g) + r^b_{T_b-1}(g))
    if (rn_out) { rno = rn_out + (row * K + lane) * (int64_t)T; rbo = rb_out + (row * K + lane) * (int64_t)T; }
  }
  for (int ci = 0; ci < nchunk; ++ci) {
    if (wid != 0) {
      if (ci + 1 < nchunk) stage(ci + 1, tid - 64, 192);
    } else if (live) {
      const float* xc = s_x[ci & 1][lane];
      const int t0 = ci * JS_TC, t1 = min(Tb, t0 + JS_TC);
      int tt = t0;
      if (ci == 0) {
        rn = n == 0 ? xc[0] : NEG_INF;
        rb = NEG_INF;
        psi = rn;
        if (rno) { js_st(rno, rn); js_st(rbo, rb); }
        tt = 1;
      }
#pragma unroll 4
      for (; tt < t1; ++tt) {
        const float p = phi[tt - 1], xv = xc[tt - t0];
        const float rn2 = js_lae(rn, p) + xv;
        const float rb2 = js_lae(rb, rn) + s_blank[tt];
        psi = js_lae(psi, p + xv);
        rn = rn2;
        rb = rb2;
        if (rno) { js_st(rno + tt, rn); js_st(rbo + tt, rb); }
      }
    }
    __syncthreads();
  }
  if (wid == 0 && lane < K) {
    s_psi[lane] = psi;
    if (psi_out) js_st(psi_out + row * K + lane, psi);
  }
  if (!k_score) return;                               // (uniform) prefix scores only
  __syncthreads();
  if (tid < K) {
    const float cs = cand_score[row * K + tid];
    float j = cs;
    if (ctc_w != 0.f) {                               // at lambda = 0 the CTC term is 0, even where psi is -inf
      const float ph = s_psi[tid];
      j = (ph == NEG_INF || psi_g == NEG_INF) ? NEG_INF : cs + ctc_w * (ph - psi_g);
    }
    if (!(j == j)) j = NEG_INF;
    s_j[tid] = j;
  }
  __syncthreads();
  if (tid < K) {
    const float j = s_j[tid];
    const int c0 = s_c[tid];
    int r = 0;
    for (int q = 0; q < K; ++q) {
      const float o = s_j[q];
      const int oc = s_c[q];
      r += o > j || (o == j && (oc < c0 || (oc == c0 && q < tid)));
    }
    if (r < beam) {
      k_score[row * beam + r] = j;
      k_idx[row * beam + r] = c0;
      k_src[row * beam + r] = (int32_t)(row * K + tid);
    }
  }
}

extern "C" int32_t otr_ctc_prefix_score(const float* log_probs, int64_t ld, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                                        int32_t blank, int32_t eos, int64_t rows, int32_t rows_per_utt, int32_t K, const int32_t* cand_idx,
                                        const float* cand_score, const uint8_t* flags, const int64_t* preds, int64_t ldp, int32_t t,
                                        const int32_t* pos, const int32_t* jsrc, const float* rn_in, const float* rb_in,
                                        const float* psi_in, float ctc_weight, float* rn_out, float* rb_out, float* psi_out,
                                        int32_t beam, float* k_score, int64_t* k_idx, int32_t* k_src, void* stream) {
  OTR_REQUIRE(log_probs && lengths && cand_idx && preds, "ctc_prefix_score: null pointer");
  OTR_REQUIRE(jsrc && rn_in && rb_in && psi_in, "ctc_prefix_score: null parent state");
  OTR_REQUIRE((rn_out == nullptr) == (rb_out == nullptr), "ctc_prefix_score: rn_out and rb_out go together");
  OTR_REQUIRE(B >= 1 && T >= 1 && T <= JS_MAXT, "ctc_prefix_score: T'=%d must be in [1, %d]", T, JS_MAXT);
  OTR_REQUIRE(V >= 1 && ld >= V && blank >= 0 && blank < V && eos >= 0 && eos < V, "ctc_prefix_score: bad V=%d / blank / eos", V);
  OTR_REQUIRE(K >= 1 && K <= JS_MAXK && K <= V, "ctc_prefix_score: K=%d must be in [1, min(%d, V=%d)]", K, JS_MAXK, V);
  OTR_REQUIRE(rows_per_utt >= 1 && rows >= 0 && rows <= (int64_t)B * rows_per_utt, "ctc_prefix_score: rows=%lld > B x rows_per_utt",
              (long long)rows);
  OTR_REQUIRE(pos || (t >= 1 && t < ldp), "ctc_prefix_score: t=%d must be in [1, ldp)", t);
  if (cand_score) {
    OTR_REQUIRE(k_score && k_idx && k_src, "ctc_prefix_score: null top-beam output");
    OTR_REQUIRE(beam >= 1 && beam <= JS_MAXBEAM && beam <= K, "ctc_prefix_score: beam=%d must be in [1, min(%d, K=%d)]", beam,
                JS_MAXBEAM, K);
    OTR_REQUIRE(ctc_weight >= 0.f && ctc_weight <= 1.f, "ctc_prefix_score: ctc_weight must be in [0, 1]");
  }
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, log_probs, ld, lengths, T, V, blank,
                     eos, rows_per_utt, K, cand_idx, cand_score, flags, preds, ldp, t, pos, jsrc, rn_in, rb_in, psi_in, ctc_weight, rn_out,
                     rb_out, psi_out, beam, cand_score ? k_score : nullptr, k_idx, k_src);
  return otr_check_launch("ctc_prefix_score");
}
