// Knowledge distillation: the temperature-scaled KL divergence of a student's logits from a teacher's, per frame, with its gradient into
// the student's logits (DistillTraining, ops.distill_loss / ops.distill_loss_topk).  include/otrans_hip.h states the semantics.  f32 in
// both builds.
//  * distill_rows:  one WAVE per row.  The dense form reads the student's and the teacher's row once, together, into online maxima / sums
//                   (rowlse.h for the student); the teacher's run also carries the cross term sum e^{b - m} (b - a), a = s / tau,
//                   b = t / tau, rescaled with the sum whenever the maximum moves, so kl = C / S_t - (m_t - m_s) - (ln S_t - ln S_s)
//                   needs no second read.  The sparse form reads the student's row once and then gathers student[r, top_idx]: the K <= 128
//                   entries are two per lane.  Every row leaves (m_s, 1 / S_s, m_t, 1 / S_t) in the workspace; 1 / S_s = -1 marks a dead row.
//  * distill_post:  ONE workgroup: thread t adds row_kl of rows t, t + 256, ... in order, one LDS tree: the same sum on every run.  It
//                   leaves the loss and the gradient's factor g tau / n_live.
//  * distill_grad:  one wave per row of dlogits.  A live row is read once more; factor (p - q) leaves with 16-byte stores where the
//                   address allows; dead rows and the columns behind V are written as zeros.  The sparse form writes factor p first and
//                   then, once those stores have landed, the listed entries again with their q.
#include <float.h>

#include "common.h"
#include "rowlse.h"

constexpr int DS_MAXV = 8192;      // the vocabulary limit of the teacher-forced scorers and of otr_ctc_topk
constexpr int DS_MAXK = 128;       // otr_ctc_topk's limit: two entries per lane

// the teacher's running maximum m, sum s of e^{b - m} and cross term c = sum of e^{b - m} (b - a) of what a lane has seen
struct DsRun { float m, s, c; };

__device__ __forceinline__ void ds_take(DsRun& r, float b, float a) {
  if (b > r.m) {                                      // new maximum: rescale (exp(-inf - b) = 0 the first time)
    const float f = __expf(r.m - b);
    r.s = r.s * f + 1.f;
    r.c = r.c * f + (b - a);
    r.m = b;
  } else if (b > NEG_INF) {                           // an element of -inf adds nothing (0 * -inf would be NaN)
    const float e = __expf(b - r.m);
    r.s += e;
    r.c += e * (b - a);
  }
}
__device__ __forceinline__ float ds_term(float b, float a, float m) { return b > NEG_INF ? __expf(b - m) * (b - a) : 0.f; }
__device__ __forceinline__ void ds_take4(DsRun& r, const float4& b, const float4& a) {
  const float mq = fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w));
  if (mq > r.m) {
    const float f = __expf(r.m - mq);
    r.s *= f;
    r.c *= f;
    r.m = mq;
  }
  if (r.m > NEG_INF) {
    r.s += __expf(b.x - r.m) + __expf(b.y - r.m) + __expf(b.z - r.m) + __expf(b.w - r.m);
    r.c += ds_term(b.x, a.x, r.m) + ds_term(b.y, a.y, r.m) + ds_term(b.z, a.z, r.m) + ds_term(b.w, a.w, r.m);
  }
}

__device__ __forceinline__ float4 ds_ld4(const float* x, int q, bool vec, float k) {      // columns 4q .. 4q + 3, times k
  float4 v;
  if (vec) v = *reinterpret_cast<const float4*>(x + 4 * q);
  else v = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
  return make_float4(v.x * k, v.y * k, v.z * k, v.w * k);
}
__device__ __forceinline__ void ds_st4(float* d, int q, bool vec, const float4& v) {
  if (vec) {
    *reinterpret_cast<float4*>(d + 4 * q) = v;
  } else {
    d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
  }
}
__device__ __forceinline__ bool ds_vec(const float* base, int64_t ld) { return ((uintptr_t)base % 16 == 0) && (ld % 4 == 0); }

// the row s[0 .. V) / tau (and, DENSE, t[0 .. V) / tau beside it) by the 64 lanes of a wave, read once, four loads in flight per lane
template <bool DENSE>
__device__ __forceinline__ void ds_row(const float* s, const float* t, int V, bool vs, bool vt, int lane, float inv_tau, RsRun& rs, DsRun& rt) {
  const int nq = V >> 2;
  int q = lane;
  if constexpr (DENSE) {
    for (; q + 64 < nq; q += 128) {
      const float4 a0 = ds_ld4(s, q, vs, inv_tau), a1 = ds_ld4(s, q + 64, vs, inv_tau);
      const float4 b0 = ds_ld4(t, q, vt, inv_tau), b1 = ds_ld4(t, q + 64, vt, inv_tau);
      rs_take4(rs, a0); rs_take4(rs, a1);
      ds_take4(rt, b0, a0); ds_take4(rt, b1, a1);
    }
    for (; q < nq; q += 64) {
      const float4 a0 = ds_ld4(s, q, vs, inv_tau), b0 = ds_ld4(t, q, vt, inv_tau);
      rs_take4(rs, a0);
      ds_take4(rt, b0, a0);
    }
    for (int v = 4 * nq + lane; v < V; v += 64) {     // the row's last, partial quad
      const float a = s[v] * inv_tau;
      rs_take(rs, a);
      ds_take(rt, t[v] * inv_tau, a);
    }
  } else {
    for (; q + 192 < nq; q += 256) {
      const float4 a0 = ds_ld4(s, q, vs, inv_tau), a1 = ds_ld4(s, q + 64, vs, inv_tau), a2 = ds_ld4(s, q + 128, vs, inv_tau),
                   a3 = ds_ld4(s, q + 192, vs, inv_tau);
      rs_take4(rs, a0); rs_take4(rs, a1); rs_take4(rs, a2); rs_take4(rs, a3);
    }
    for (; q < nq; q += 64) rs_take4(rs, ds_ld4(s, q, vs, inv_tau));
    for (int v = 4 * nq + lane; v < V; v += 64) rs_take(rs, s[v] * inv_tau);
  }
}

// entry k of a sparse teacher row: listed iff k < K and 0 <= top_idx < V; then b = top_val / tau and idx, else b = -inf and idx = -1
__device__ __forceinline__ void ds_entry(const float* top_val, const int32_t* top_idx, int64_t row, int K, int k, int V, float inv_tau,
                                         float& b, int& idx) {
  b = NEG_INF;
  idx = -1;
  if (k < K) {
    const int t = top_idx[row * K + k];
    if (t >= 0 && t < V) {
      idx = t;
      b = top_val[row * K + k] * inv_tau;
    }
  }
}

// ---------------------------------------------------------------- rows
__global__ __launch_bounds__(256) void distill_rows_kernel(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t,
                                                           const float* top_val, const int32_t* top_idx, int K, const int32_t* lengths,
                                                           int64_t rows, int T, int V, float inv_tau, float* row_kl, float4* stats) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  const int64_t b = row / T;
  const int i = (int)(row - b * T);
  float kl = 0.f;
  float4 st = make_float4(0.f, -1.f, 0.f, 0.f);        // 1 / S_s = -1: a dead row
  if (i < min(max(lengths[b], 0), T)) {
    const float* s = student + row * ld_s;
    const bool vs = ds_vec(student, ld_s);
    RsRun rs{NEG_INF, 0.f};
    DsRun rt{NEG_INF, 0.f, 0.f};
    float Mt, St, Ct;
    bool any;
    if (teacher) {
      ds_row<true>(s, teacher + row * ld_t, V, vs, ds_vec(teacher, ld_t), lane, inv_tau, rs, rt);
      Mt = wave_max(rt.m);
      const float f = rt.m > NEG_INF ? __expf(rt.m - Mt) : 0.f;
      St = wave_sum(rt.s * f);
      Ct = wave_sum(rt.c * f);
      any = Mt > NEG_INF;                              // a teacher row of -inf throughout has no distribution: dead
    } else {
      ds_row<false>(s, nullptr, V, vs, false, lane, inv_tau, rs, rt);
      float b0, b1;
      int i0, i1;
      ds_entry(top_val, top_idx, row, K, lane, V, inv_tau, b0, i0);
      ds_entry(top_val, top_idx, row, K, lane + 64, V, inv_tau, b1, i1);
      const float a0 = i0 >= 0 ? s[i0] * inv_tau : 0.f, a1 = i1 >= 0 ? s[i1] * inv_tau : 0.f;
      Mt = wave_max(fmaxf(b0, b1));
      any = Mt > NEG_INF;                              // no listed entry (or -inf in all of them): dead
      const float e0 = any && b0 > NEG_INF ? __expf(b0 - Mt) : 0.f, e1 = any && b1 > NEG_INF ? __expf(b1 - Mt) : 0.f;
      St = wave_sum(e0 + e1);
      Ct = wave_sum((e0 != 0.f ? e0 * (b0 - a0) : 0.f) + (e1 != 0.f ? e1 * (b1 - a1) : 0.f));
    }
    if (any) {
      const float Ms = wave_max(rs.m);
      const float Ss = wave_sum(rs.m > NEG_INF ? rs.s * __expf(rs.m - Ms) : 0.f);
      // sum q (b - a) - (lse_t - lse_s), the difference of the logsumexps formed from small terms
      kl = Ct / St - ((Mt - Ms) + (logf(St) - logf(Ss)));
      st = make_float4(Ms, 1.f / Ss, Mt, 1.f / St);
    }
  }
  if (lane == 0) {
    row_kl[row] = kl;
    stats[row] = st;
  }
}

// ---------------------------------------------------------------- loss, n_live, g tau / n_live
__global__ __launch_bounds__(256) void distill_post_kernel(const float* row_kl, const float4* stats, int64_t rows, float tau,
                                                           const float* grad_scale, float* loss, float* coef) {
  __shared__ float s_sum[256];
  __shared__ int s_cnt[256];
  const int tid = threadIdx.x;
  float sum = 0.f;
  int cnt = 0;
  for (int64_t r = tid; r < rows; r += 256)
    if (stats[r].y >= 0.f) {
      sum += row_kl[r];
      ++cnt;
    }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                 // one tree, the same order on every run
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int n_live = s_cnt[0];
    const float g = grad_scale ? *grad_scale : 1.f;
    *loss = n_live > 0 ? tau * tau * s_sum[0] / (float)n_live : 0.f;
    *coef = n_live > 0 ? g * tau / (float)n_live : 0.f;
  }
}

// ---------------------------------------------------------------- gradient
// c (p - q) of four columns: p = e^{a - m_s} / S_s, q = e^{b - m_t} / S_t (an element of -inf gives 0)
__device__ __forceinline__ float4 ds_grad4(const float4& a, const float4& b, const float4& st, float c) {
  return make_float4(c * (expf(a.x - st.x) * st.y - expf(b.x - st.z) * st.w), c * (expf(a.y - st.x) * st.y - expf(b.y - st.z) * st.w),
                     c * (expf(a.z - st.x) * st.y - expf(b.z - st.z) * st.w), c * (expf(a.w - st.x) * st.y - expf(b.w - st.z) * st.w));
}
__device__ __forceinline__ float4 ds_p4(const float4& a, const float4& st, float c) {
  const float k = c * st.y;
  return make_float4(k * expf(a.x - st.x), k * expf(a.y - st.x), k * expf(a.z - st.x), k * expf(a.w - st.x));
}

__global__ __launch_bounds__(256) void distill_grad_kernel(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t,
                                                           const float* top_val, const int32_t* top_idx, int K, int64_t rows, int V,
                                                           float inv_tau, const float4* stats, const float* coef, float* dlogits,
                                                           int64_t ld_d) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  float* d = dlogits + row * ld_d;
  const bool vout = ds_vec(dlogits, ld_d);
  const float4 st = stats[row];
  if (st.y < 0.f) {                                   // a dead row: zeros, nothing of it is read
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vout) {
      for (int q = lane; q < (int)(ld_d >> 2); q += 64) ds_st4(d, q, true, zero);
    } else {
      for (int64_t v = lane; v < ld_d; v += 64) d[v] = 0.f;
    }
    return;
  }
  const float c = *coef;
  const float* s = student + row * ld_s;
  const bool vs = ds_vec(student, ld_s);
  const int nq = V >> 2;
  int q = lane;
  if (teacher) {
    const float* t = teacher + row * ld_t;
    const bool vt = ds_vec(teacher, ld_t);
    for (; q + 64 < nq; q += 128) {                   // four loads in flight per lane
      const float4 a0 = ds_ld4(s, q, vs, inv_tau), a1 = ds_ld4(s, q + 64, vs, inv_tau);
      const float4 b0 = ds_ld4(t, q, vt, inv_tau), b1 = ds_ld4(t, q + 64, vt, inv_tau);
      ds_st4(d, q, vout, ds_grad4(a0, b0, st, c));
      ds_st4(d, q + 64, vout, ds_grad4(a1, b1, st, c));
    }
    for (; q < nq; q += 64) ds_st4(d, q, vout, ds_grad4(ds_ld4(s, q, vs, inv_tau), ds_ld4(t, q, vt, inv_tau), st, c));
    for (int v = 4 * nq + lane; v < V; v += 64)       // the row's last, partial quad
      d[v] = c * (expf(s[v] * inv_tau - st.x) * st.y - expf(t[v] * inv_tau - st.z) * st.w);
    for (int64_t v = V + lane; v < ld_d; v += 64) d[v] = 0.f;       // the padding behind the vocabulary
    return;
  }
  for (; q + 192 < nq; q += 256) {
    const float4 a0 = ds_ld4(s, q, vs, inv_tau), a1 = ds_ld4(s, q + 64, vs, inv_tau), a2 = ds_ld4(s, q + 128, vs, inv_tau),
                 a3 = ds_ld4(s, q + 192, vs, inv_tau);
    ds_st4(d, q, vout, ds_p4(a0, st, c));
    ds_st4(d, q + 64, vout, ds_p4(a1, st, c));
    ds_st4(d, q + 128, vout, ds_p4(a2, st, c));
    ds_st4(d, q + 192, vout, ds_p4(a3, st, c));
  }
  for (; q < nq; q += 64) ds_st4(d, q, vout, ds_p4(ds_ld4(s, q, vs, inv_tau), st, c));
  for (int v = 4 * nq + lane; v < V; v += 64) d[v] = c * st.y * expf(s[v] * inv_tau - st.x);
  for (int64_t v = V + lane; v < ld_d; v += 64) d[v] = 0.f;
  // the listed entries once more, with their q: other lanes of this wave wrote these addresses above, so those stores land first
  wait_vm<0>();
  for (int k = lane; k < K; k += 64) {
    float b;
    int idx;
    ds_entry(top_val, top_idx, row, K, k, V, inv_tau, b, idx);
    if (idx >= 0) {
      const float qk = b > NEG_INF ? expf(b - st.z) * st.w : 0.f;
      d[idx] = c * (expf(s[idx] * inv_tau - st.x) * st.y - qk);
    }
  }
}

// ---------------------------------------------------------------- entries
static bool distill_shape_ok(int64_t B, int64_t T) { return B >= 0 && T >= 1 && B * T < (1ll << 30); }

extern "C" int64_t otr_distill_workspace_floats(int32_t B, int32_t T) {
  if (!distill_shape_ok(B, T)) return -1;
  return 4 * (int64_t)B * T + 4;                      // (m_s, 1 / S_s, m_t, 1 / S_t) of every row, then g tau / n_live
}

extern "C" int32_t otr_distill_loss(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const float* top_val,
                                    const int32_t* top_idx, int32_t K, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                                    float temperature, const float* grad_scale, float* loss, float* row_kl, float* dlogits, int64_t ld_d,
                                    float* workspace, int64_t workspace_floats, void* stream) {
  const bool sparse = top_val || top_idx || K != 0;
  OTR_REQUIRE((teacher != nullptr) != sparse, "distill_loss: give the dense teacher or the sparse one (top_val, top_idx, K), not %s",
              teacher ? "both" : "neither");
  OTR_REQUIRE(V >= 1 && V <= DS_MAXV && ld_s >= V, "distill_loss: V=%d must be in [1, %d], ld_s=%lld >= V", V, DS_MAXV, (long long)ld_s);
  OTR_REQUIRE(sparse || ld_t >= V, "distill_loss: ld_t=%lld < V=%d", (long long)ld_t, V);
  OTR_REQUIRE(!sparse || (K >= 1 && K <= DS_MAXK), "distill_loss: K=%d entries per row, 1 .. %d supported", K, DS_MAXK);
  OTR_REQUIRE(distill_shape_ok(B, T), "distill_loss: bad shape B=%d T=%d (T >= 1, B*T < 2^30)", B, T);
  OTR_REQUIRE(!dlogits || ld_d >= V, "distill_loss: ld_d=%lld < V=%d", (long long)ld_d, V);
  OTR_REQUIRE(temperature > 0.f && temperature <= FLT_MAX, "distill_loss: temperature=%g must be finite and > 0", (double)temperature);
  if (B == 0) return 0;
  OTR_REQUIRE(student && lengths && loss && row_kl && (!sparse || (top_val && top_idx)), "distill_loss: null pointer");
  const int64_t rows = (int64_t)B * T;
  OTR_REQUIRE(workspace && workspace_floats >= 4 * rows + 4, "distill_loss: workspace of %lld floats, %lld needed", (long long)workspace_floats,
              (long long)(4 * rows + 4));
  OTR_REQUIRE((uintptr_t)workspace % 16 == 0, "distill_loss: the workspace must be 16-byte aligned");
  float4* stats = reinterpret_cast<float4*>(workspace);
  float* coef = workspace + 4 * rows;
  const float inv_tau = 1.f / temperature;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipLaunchKernelGGL(distill_rows_kernel, grid, dim3(256), 0, s, student, ld_s, teacher, ld_t, top_val, top_idx, K, lengths, rows, T, V, inv_tau,
                     row_kl, stats);
  hipLaunchKernelGGL(distill_post_kernel, dim3(1), dim3(256), 0, s, (const float*)row_kl, (const float4*)stats, rows, temperature, grad_scale,
                     loss, coef);
  if (dlogits)
    hipLaunchKernelGGL(distill_grad_kernel, grid, dim3(256), 0, s, student, ld_s, teacher, ld_t, top_val, top_idx, K, rows, V, inv_tau,
                       (const float4*)stats, (const float*)coef, dlogits, ld_d);
  return otr_check_launch("distill_loss");
}
