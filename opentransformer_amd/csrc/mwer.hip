// Minimum word error rate (MWER) training: the N-best approximation of the expected number of errors with its gradient into the
// decoder's logits (MWERTraining, ops.mwer_loss).  include/otrans_hip.h states the semantics.  f32 in both builds.
//  * mwer_rows:  otr_rescore_score's row pass -- one workgroup per slot, one WAVE per row, the row read once (16-byte loads where its
//                address allows) into an online max / sum (rowlse.h) -- that also leaves every row's logsumexp in the workspace.  Wave w
//                adds up rows w, w + 4, ... in order and thread 0 adds the four partials in order: the same sum on every run.  A slot
//                without rows, with errors < 0 or with a target outside [0, V) leaves s = -inf: that is how the next two launches
//                know a dead slot.
//  * mwer_post:  ONE workgroup over the B x N scalars: thread t takes utterances t, t + 256, ... (softmax over the live slots, E_b),
//                the sums over the utterances go through one LDS tree, then every thread forms g c_h of its utterances.
//  * mwer_grad:  one wave per row of dlogits.  A live row is read once more, g c_h (1[v == target] - exp(x - lse)) leaves with
//                16-byte stores where the address allows; every other row, and the columns behind V, are written as zeros.
#include "common.h"
#include "rowlse.h"

constexpr int MW_MAXN = 32;        // hypotheses per utterance (the edit distance's and the rescoring's limit)
constexpr int MW_MAXV = 8192;      // the rescoring's vocabulary limit

// ---------------------------------------------------------------- rows
__global__ __launch_bounds__(256) void mwer_rows_kernel(const float* logits, int64_t ld, const int64_t* ys_out, int64_t ldt,
                                                        const int32_t* n_rows, const int32_t* errors, int max_len, int V, float* seq_logp,
                                                        float* lse) {
  __shared__ float part[4];
  __shared__ int bad[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t h = blockIdx.x;
  const int n = min(max(n_rows[h], 0), max_len);
  if (n == 0 || errors[h] < 0) {                      // nothing of the slot is read
    if (tid == 0) seq_logp[h] = NEG_INF;
    return;
  }
  const bool vec = ((uintptr_t)logits % 16 == 0) && (ld % 4 == 0);     // every row starts on a 16-byte boundary
  float acc = 0.f;
  int wrong = 0;
  for (int l = wid; l < n; l += 4) {
    const float* x = logits + (h * max_len + l) * ld;
    float M, S;
    rs_row(x, V, vec, lane, M, S);
    const float z = M + __logf(S);
    if (lane == 0) lse[h * max_len + l] = z;
    const int64_t t = ys_out[h * ldt + l];
    if (t >= 0 && t < V) acc += x[t] - z;
    else wrong = 1;                                   // a target outside the vocabulary: the slot is dead
  }
  if (lane == 0) {
    part[wid] = acc;
    bad[wid] = wrong;
  }
  __syncthreads();
  if (tid == 0) seq_logp[h] = (bad[0] | bad[1] | bad[2] | bad[3]) ? NEG_INF : ((part[0] + part[1]) + part[2]) + part[3];
}

// ---------------------------------------------------------------- posteriors, expected errors, loss, g c_h
__global__ __launch_bounds__(256) void mwer_post_kernel(const float* seq_logp, const int32_t* errors, int B, int N, const float* grad_scale,
                                                        float* loss, float* post, float* utt_err, float* cg) {
  __shared__ float s_sum[256];
  __shared__ int s_cnt[256];
  const int tid = threadIdx.x;
  float esum = 0.f;
  int cnt = 0;
  for (int b = tid; b < B; b += 256) {
    const float* s = seq_logp + (int64_t)b * N;
    const int32_t* w = errors + (int64_t)b * N;
    float* p = post + (int64_t)b * N;
    float m = NEG_INF;
    bool any = false;
    for (int n = 0; n < N; ++n)
      if (!(s[n] == NEG_INF)) {
        m = fmaxf(m, s[n]);
        any = true;
      }
    float z = 0.f;
    for (int n = 0; n < N; ++n)
      if (!(s[n] == NEG_INF)) z += expf(s[n] - m);
    float e = 0.f;
    for (int n = 0; n < N; ++n) {
      const float pn = !(s[n] == NEG_INF) ? expf(s[n] - m) / z : 0.f;
      p[n] = pn;
      if (pn != 0.f) e += pn * (float)w[n];
    }
    utt_err[b] = e;
    if (any) {
      esum += e;
      ++cnt;
    }
  }
  s_sum[tid] = esum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                 // one tree, the same order on every run
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
    }
    __syncthreads();
  }
  const int b_live = s_cnt[0];
  if (tid == 0) *loss = b_live > 0 ? s_sum[0] / (float)b_live : 0.f;
  if (!cg) return;
  const float g = grad_scale ? *grad_scale : 1.f;
  for (int b = tid; b < B; b += 256) {                // this thread wrote post and utt_err of these utterances
    const float e = utt_err[b];
    for (int n = 0; n < N; ++n) {
      const int64_t h = (int64_t)b * N + n;
      const float pn = post[h];
      cg[h] = pn != 0.f ? g * (pn * ((float)errors[h] - e) / (float)b_live) : 0.f;
    }
  }
}

// ---------------------------------------------------------------- gradient
__device__ __forceinline__ float4 mw_ld4(const float* x, int q, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(x + 4 * q);
  return make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}
__device__ __forceinline__ void mw_st4(float* d, int q, bool vec, const float4& v) {
  if (vec) {
    *reinterpret_cast<float4*>(d + 4 * q) = v;
  } else {
    d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
  }
}
// g c_h (1[v == t] - softmax(x)_v) of columns 4q .. 4q + 3
__device__ __forceinline__ float4 mw_grad4(const float4& a, int q, int t, float z, float c) {
  const int v = 4 * q;
  return make_float4(c * ((v == t ? 1.f : 0.f) - __expf(a.x - z)), c * ((v + 1 == t ? 1.f : 0.f) - __expf(a.y - z)),
                     c * ((v + 2 == t ? 1.f : 0.f) - __expf(a.z - z)), c * ((v + 3 == t ? 1.f : 0.f) - __expf(a.w - z)));
}

__global__ __launch_bounds__(256) void mwer_grad_kernel(const float* logits, int64_t ld, const int64_t* ys_out, int64_t ldt,
                                                        const int32_t* n_rows, int64_t rows, int max_len, int V, const float* seq_logp,
                                                        const float* lse, const float* cg, float* dlogits, int64_t ldd) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wid;
  if (row >= rows) return;
  const int64_t h = row / max_len;
  const int l = (int)(row - h * max_len);
  float* d = dlogits + row * ldd;
  const bool vout = ((uintptr_t)dlogits % 16 == 0) && (ldd % 4 == 0);
  const float c = cg[h];
  if (l >= min(max(n_rows[h], 0), max_len) || seq_logp[h] == NEG_INF || c == 0.f) {    // no gradient here: zeros, the row is not read
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vout) {
      for (int q = lane; q < (int)(ldd >> 2); q += 64) mw_st4(d, q, true, zero);
    } else {
      for (int64_t v = lane; v < ldd; v += 64) d[v] = 0.f;
    }
    return;
  }
  const float* x = logits + row * ld;
  const bool vin = ((uintptr_t)logits % 16 == 0) && (ld % 4 == 0);
  const int t = (int)ys_out[h * ldt + l];             // inside [0, V): the slot is live
  const float z = lse[row];
  const int nq = V >> 2;
  int q = lane;
  for (; q + 192 < nq; q += 256) {                    // four loads in flight per lane
    const float4 a0 = mw_ld4(x, q, vin), a1 = mw_ld4(x, q + 64, vin), a2 = mw_ld4(x, q + 128, vin), a3 = mw_ld4(x, q + 192, vin);
    mw_st4(d, q, vout, mw_grad4(a0, q, t, z, c));
    mw_st4(d, q + 64, vout, mw_grad4(a1, q + 64, t, z, c));
    mw_st4(d, q + 128, vout, mw_grad4(a2, q + 128, t, z, c));
    mw_st4(d, q + 192, vout, mw_grad4(a3, q + 192, t, z, c));
  }
  for (; q < nq; q += 64) mw_st4(d, q, vout, mw_grad4(mw_ld4(x, q, vin), q, t, z, c));
  for (int v = 4 * nq + lane; v < V; v += 64) d[v] = c * ((v == t ? 1.f : 0.f) - __expf(x[v] - z));    // the row's last, partial quad
  for (int64_t v = V + lane; v < ldd; v += 64) d[v] = 0.f;                                             // the padding behind the vocabulary
}

// ---------------------------------------------------------------- entries
static bool mwer_shape_ok(int64_t B, int64_t N, int64_t max_len) {
  return B >= 0 && N >= 1 && N <= MW_MAXN && max_len >= 1 && B * N * max_len < (1ll << 30);
}

extern "C" int64_t otr_mwer_workspace_floats(int32_t B, int32_t N, int32_t max_len) {
  if (!mwer_shape_ok(B, N, max_len)) return -1;
  return (int64_t)B * N * max_len + (int64_t)B * N;   // every row's logsumexp, then g c_h of every slot
}

extern "C" int32_t otr_mwer_loss(const float* logits, int64_t ld, const int64_t* ys_out, int64_t ld_ys, const int32_t* n_rows,
                                 const int32_t* errors, int32_t B, int32_t N, int32_t max_len, int32_t V, const float* grad_scale,
                                 float* loss, float* seq_logp, float* post, float* utt_err, float* dlogits, int64_t ld_dlogits,
                                 float* workspace, int64_t workspace_floats, void* stream) {
  OTR_REQUIRE(N >= 1 && N <= MW_MAXN, "mwer_loss: N=%d hypotheses per utterance, 1 .. %d supported", N, MW_MAXN);
  OTR_REQUIRE(V >= 1 && V <= MW_MAXV && ld >= V, "mwer_loss: V=%d must be in [1, %d], ld >= V", V, MW_MAXV);
  OTR_REQUIRE(mwer_shape_ok(B, N, max_len) && ld_ys >= max_len, "mwer_loss: bad shape B=%d N=%d max_len=%d ld_ys=%lld (B*N*max_len < 2^30)", B,
              N, max_len, (long long)ld_ys);
  OTR_REQUIRE(!dlogits || ld_dlogits >= V, "mwer_loss: ld_dlogits=%lld < V=%d", (long long)ld_dlogits, V);
  if (B == 0) return 0;
  OTR_REQUIRE(logits && ys_out && n_rows && errors && loss && seq_logp && post && utt_err, "mwer_loss: null pointer");
  const int64_t nh = (int64_t)B * N, rows = nh * max_len;
  OTR_REQUIRE(workspace && workspace_floats >= rows + nh, "mwer_loss: workspace of %lld floats, %lld needed", (long long)workspace_floats,
              (long long)(rows + nh));
  float* lse = workspace;
  float* cg = workspace + rows;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mwer_rows_kernel, dim3((unsigned)nh), dim3(256), 0, s, logits, ld, ys_out, ld_ys, n_rows, errors, max_len, V, seq_logp, lse);
  hipLaunchKernelGGL(mwer_post_kernel, dim3(1), dim3(256), 0, s, (const float*)seq_logp, errors, B, N, grad_scale, loss, post, utt_err,
                     dlogits ? cg : (float*)nullptr);
  if (dlogits)
    hipLaunchKernelGGL(mwer_grad_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, ld, ys_out, ld_ys, n_rows, rows, max_len, V,
                       (const float*)seq_logp, (const float*)lse, (const float*)cg, dlogits, ld_dlogits);
  return otr_check_launch("mwer_loss");
}
