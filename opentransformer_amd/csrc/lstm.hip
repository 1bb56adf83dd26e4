// Training the recurrent language model (model/lm.py:33-91 through nn.LSTM's backward): the per-step kernels of the forward pass
// that keeps what backpropagation through time needs, and of that backward pass.  include/otrans_hip.h states the semantics and
// the limits.  The input projections of all steps and the weight gradients are GEMMs of the existing otr_linear_* launches; what
// is here is the strictly sequential part.
//  * lstm_pack_whh:      W_hh [4H, H] f32 -> two MFMA-fragment-ordered copies in the compute type: per 16-unit block the four gate
//                        rows of those units (forward operand) and the 16 columns of those units (backward operand), each k-step's
//                        64 chunks contiguous, so a wave reads 1 KiB per k-step and a workgroup reads only its own share.
//  * lstm_fwd_step:      one launch per (layer, t).  Workgroup = 16 hidden units x all rows x all four gates: wave (gate, K half)
//                        contracts h_{t-1} with its gate rows, the partials meet in LDS, the cell update is local to the block.
//  * lstm_bwd_step:      one launch per (layer, t), t descending.  dh_t = dy_t + dG_{t+1} W_hh restricted to the block (8 waves split
//                        the 4H contraction), then the cell backward writes dG_t (all four gates of the block) and dc_{t-1}.
//  * lstm_cell_fwd/bwd:  the same cell math on rows of gate sums made elsewhere: the unfused route (shapes outside the limits) whose
//                        recurrent products are otr_linear_fwd / otr_linear_dgrad calls.
#include "common.h"

constexpr int LS_HB = 16;     // hidden units per workgroup (one MFMA column tile)
constexpr int LS_NT = 512;    // threads of a step workgroup: 8 waves
constexpr int LS_MT = OTR_LSTM_MAX_ROWS / 16;

__device__ __forceinline__ float ls_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// gate pre-activations (i, f, g, o) -> activations, c, h.  Same expressions as otr_lstm_cell.
__device__ __forceinline__ void ls_cell_fwd(const float* z, float cp, float* a, float& cn, float& hn) {
  a[0] = ls_sigmoid(z[0]);
  a[1] = ls_sigmoid(z[1]);
  a[2] = tanhf(z[2]);
  a[3] = ls_sigmoid(z[3]);
  cn = a[1] * cp + a[0] * a[2];
  hn = a[3] * tanhf(cn);
}

// dh (total gradient into h_t), dc_next (from step t+1), activations, c_t, c_{t-1} -> gate gradients dz, dc_{t-1}
__device__ __forceinline__ void ls_cell_bwd(float dh, float dcn, const float* a, float c, float cp, float* dz, float& dcp) {
  const float tc = tanhf(c);
  const float dc = dh * a[3] * (1.f - tc * tc) + dcn;
  dz[0] = dc * a[2] * a[0] * (1.f - a[0]);
  dz[1] = dc * cp * a[1] * (1.f - a[1]);
  dz[2] = dc * a[0] * (1.f - a[2] * a[2]);
  dz[3] = dh * tc * a[3] * (1.f - a[3]);
  dcp = dc * a[1];
}

template <class CT> __device__ __forceinline__ void ls_store(CT* p, float v);
template <> __device__ __forceinline__ void ls_store<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void ls_store<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

// ---------------------------------------------------------------- W_hh packs
template <class CT>
__global__ void lstm_pack_kernel(const float* __restrict__ w, CT* __restrict__ fwd, CT* __restrict__ bwd, int H) {
  constexpr int CE = MMA<CT>::CE, KS = MMA<CT>::KSTEP;
  const int64_t nchunk = (int64_t)4 * H * H / CE;
  const int NS = H / KS, NSB = 4 * H / KS;
  for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < nchunk; ci += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(ci & 63);
    const int64_t rest = ci >> 6;
    if (fwd) {            // chunk ((jb*4 + q)*NS + s)*64 + lane = W[q*H + jb*16 + (lane&15)][s*KS + (lane>>4)*CE + e]
      const int s = (int)(rest % NS), q = (int)((rest / NS) & 3), jb = (int)(rest / NS / 4);
      const float* src = w + (int64_t)(q * H + jb * LS_HB + (lane & 15)) * H + s * KS + (lane >> 4) * CE;
#pragma unroll
      for (int e = 0; e < CE; ++e) ls_store<CT>(fwd + ci * CE + e, src[e]);
    }
    if (bwd) {            // chunk (jb*NSB + s)*64 + lane = W[s*KS + (lane>>4)*CE + e][jb*16 + (lane&15)]
      const int s = (int)(rest % NSB), jb = (int)(rest / NSB);
      const float* src = w + (int64_t)(s * KS + (lane >> 4) * CE) * H + jb * LS_HB + (lane & 15);
#pragma unroll
      for (int e = 0; e < CE; ++e) ls_store<CT>(bwd + ci * CE + e, src[(int64_t)e * H]);
    }
  }
}

// ---------------------------------------------------------------- forward step
template <class CT>
__global__ __launch_bounds__(LS_NT) void lstm_fwd_step_kernel(const float* __restrict__ gx, const float* __restrict__ bias,
                                                              const CT* __restrict__ hprev, const float* __restrict__ cprev,
                                                              const uint4* __restrict__ wp, float* __restrict__ h,
                                                              bf16_t* __restrict__ hlp, float* __restrict__ c,
                                                              float* __restrict__ act, int B, int H) {
  __shared__ float part[2][4][OTR_LSTM_MAX_ROWS][LS_HB + 1];
  constexpr int CE = MMA<CT>::CE, KS = MMA<CT>::KSTEP;
  const int jb = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = w & 3, kh = w >> 2;
  const int NS = H / KS, nsh = NS / 2;
  const int MT = (B + 15) / 16;
  f32x4 acc[LS_MT];
#pragma unroll
  for (int m = 0; m < LS_MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (hprev) {
    const uint4* wq = wp + (int64_t)(jb * 4 + q) * NS * 64 + lane;
    for (int s = kh * nsh; s < (kh + 1) * nsh; ++s) {
      const uint4 bw = wq[(int64_t)s * 64];
      const int k = s * KS + (lane >> 4) * CE;
#pragma unroll
      for (int m = 0; m < LS_MT; ++m) {
        if (m < MT) {
          const int r = m * 16 + (lane & 15);
          const uint4 a = r < B ? *(const uint4*)(hprev + (int64_t)r * H + k) : make_uint4(0u, 0u, 0u, 0u);
          MMA<CT>::mma(acc[m], a, bw);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < LS_MT; ++m)
    if (m < MT)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[kh][q][m * 16 + (lane >> 4) * 4 + i][lane & 15] = acc[m][i];
  __syncthreads();
  for (int idx = threadIdx.x; idx < B * LS_HB; idx += LS_NT) {
    const int b = idx / LS_HB, jj = idx % LS_HB, j = jb * LS_HB + jj;
    float z[4], a[4], cn, hn;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v = gx[(int64_t)b * 4 * H + g * H + j];
      if (bias) v += bias[g * H + j];
      z[g] = v + (part[0][g][b][jj] + part[1][g][b][jj]);
    }
    ls_cell_fwd(z, cprev ? cprev[(int64_t)b * H + j] : 0.f, a, cn, hn);
    c[(int64_t)b * H + j] = cn;
    h[(int64_t)b * H + j] = hn;
    if (hlp) hlp[(int64_t)b * H + j] = f2bf(hn);
#pragma unroll
    for (int g = 0; g < 4; ++g) act[(int64_t)b * 4 * H + g * H + j] = a[g];
  }
}

// ---------------------------------------------------------------- backward step
// dcin / dcout may be the same buffer: every element is read and written by one thread, in that order.
template <class CT>
__global__ __launch_bounds__(LS_NT) void lstm_bwd_step_kernel(const float* __restrict__ dy, const CT* __restrict__ dgn,
                                                              const uint4* __restrict__ wp, const float* __restrict__ act,
                                                              const float* __restrict__ c, const float* __restrict__ cprev,
                                                              const float* dcin, float* dcout, CT* __restrict__ dg, int B, int H) {
  __shared__ float part[8][OTR_LSTM_MAX_ROWS][LS_HB + 1];
  constexpr int CE = MMA<CT>::CE, KS = MMA<CT>::KSTEP;
  const int jb = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int NSB = 4 * H / KS, nsw = NSB / 8;
  const int MT = (B + 15) / 16;
  f32x4 acc[LS_MT];
#pragma unroll
  for (int m = 0; m < LS_MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (dgn) {
    const uint4* wq = wp + (int64_t)jb * NSB * 64 + lane;
    for (int s = w * nsw; s < (w + 1) * nsw; ++s) {
      const uint4 bw = wq[(int64_t)s * 64];
      const int n = s * KS + (lane >> 4) * CE;
#pragma unroll
      for (int m = 0; m < LS_MT; ++m) {
        if (m < MT) {
          const int r = m * 16 + (lane & 15);
          const uint4 a = r < B ? *(const uint4*)(dgn + (int64_t)r * 4 * H + n) : make_uint4(0u, 0u, 0u, 0u);
          MMA<CT>::mma(acc[m], a, bw);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < LS_MT; ++m)
    if (m < MT)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[w][m * 16 + (lane >> 4) * 4 + i][lane & 15] = acc[m][i];
  __syncthreads();
  for (int idx = threadIdx.x; idx < B * LS_HB; idx += LS_NT) {
    const int b = idx / LS_HB, jj = idx % LS_HB, j = jb * LS_HB + jj;
    const int64_t o = (int64_t)b * H + j;
    float dh = 0.f;
#pragma unroll
    for (int v = 0; v < 8; ++v) dh += part[v][b][jj];
    dh += dy[o];
    float a[4], dz[4], dcp;
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = act[(int64_t)b * 4 * H + g * H + j];
    ls_cell_bwd(dh, dcin ? dcin[o] : 0.f, a, c[o], cprev ? cprev[o] : 0.f, dz, dcp);
    dcout[o] = dcp;
#pragma unroll
    for (int g = 0; g < 4; ++g) ls_store<CT>(dg + (int64_t)b * 4 * H + g * H + j, dz[g]);
  }
}

// ---------------------------------------------------------------- unfused cell (elementwise)
__global__ void lstm_cell_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ gh, const float* __restrict__ bias,
                                     const float* __restrict__ cprev, float* __restrict__ h, bf16_t* __restrict__ hlp,
                                     float* __restrict__ c, float* __restrict__ act, int64_t rows, int H) {
  const int64_t total = rows * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    float z[4], a[4], cn, hn;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v = gx[r * 4 * H + g * H + j];
      if (bias) v += bias[g * H + j];
      z[g] = gh ? v + gh[r * 4 * H + g * H + j] : v;
    }
    ls_cell_fwd(z, cprev ? cprev[i] : 0.f, a, cn, hn);
    c[i] = cn;
    h[i] = hn;
    if (hlp) hlp[i] = f2bf(hn);
#pragma unroll
    for (int g = 0; g < 4; ++g) act[r * 4 * H + g * H + j] = a[g];
  }
}

template <class CT>
__global__ void lstm_cell_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dhr, const float* __restrict__ act,
                                     const float* __restrict__ c, const float* __restrict__ cprev, const float* dcin, float* dcout,
                                     CT* __restrict__ dg, int64_t rows, int H) {
  const int64_t total = rows * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    float a[4], dz[4], dcp;
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = act[r * 4 * H + g * H + j];
    const float dh = dhr ? dy[i] + dhr[i] : dy[i];
    ls_cell_bwd(dh, dcin ? dcin[i] : 0.f, a, c[i], cprev ? cprev[i] : 0.f, dz, dcp);
    dcout[i] = dcp;
#pragma unroll
    for (int g = 0; g < 4; ++g) ls_store<CT>(dg + r * 4 * H + g * H + j, dz[g]);
  }
}

// ---------------------------------------------------------------- host entry points
static bool ls_fused_shape(int64_t rows, int32_t hidden) {
  return rows >= 1 && rows <= OTR_LSTM_MAX_ROWS && hidden >= OTR_LSTM_HIDDEN_MULT && hidden <= OTR_LSTM_MAX_HIDDEN &&
         hidden % OTR_LSTM_HIDDEN_MULT == 0;
}

extern "C" int32_t otr_lstm_step_supported(int64_t rows, int32_t hidden) { return ls_fused_shape(rows, hidden) ? 1 : 0; }

extern "C" int32_t otr_lstm_pack_whh(const float* w_hh, void* fwd_pack, void* bwd_pack, int32_t dtype, int32_t hidden, void* stream) {
  OTR_REQUIRE(w_hh && (fwd_pack || bwd_pack), "lstm_pack_whh: null pointer");
  OTR_REQUIRE(dtype == OTR_F32 || dtype == OTR_H16, "lstm_pack_whh: dtype must be OTR_F32 or this build's 16-bit type");
  OTR_REQUIRE(ls_fused_shape(1, hidden), "lstm_pack_whh: hidden %d outside the step kernels' limits", hidden);
  const int64_t nchunk = (int64_t)4 * hidden * hidden / (dtype == OTR_F32 ? 4 : 8);
  const int64_t g = (nchunk + 255) / 256;
  const dim3 grid((unsigned)(g > 8192 ? 8192 : g));
  if (dtype == OTR_F32)
    hipLaunchKernelGGL(lstm_pack_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, w_hh, (float*)fwd_pack, (float*)bwd_pack, hidden);
  else
    hipLaunchKernelGGL(lstm_pack_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, w_hh, (bf16_t*)fwd_pack, (bf16_t*)bwd_pack,
                       hidden);
  return otr_check_launch("lstm_pack_whh");
}

extern "C" int32_t otr_lstm_fwd_step(const float* gx, const float* bias, const void* h_prev, const float* c_prev, const void* fwd_pack,
                                     float* h, void* h_bf16, float* c, float* act, int32_t dtype, int64_t rows, int32_t hidden,
                                     void* stream) {
  OTR_REQUIRE(gx && fwd_pack && h && c && act, "lstm_fwd_step: null pointer");
  OTR_REQUIRE(dtype == OTR_F32 || dtype == OTR_H16, "lstm_fwd_step: dtype must be OTR_F32 or this build's 16-bit type");
  OTR_REQUIRE(ls_fused_shape(rows, hidden), "lstm_fwd_step: rows %lld / hidden %d outside the limits", (long long)rows, hidden);
  OTR_REQUIRE(((uintptr_t)h_prev & 15) == 0 && ((uintptr_t)fwd_pack & 15) == 0, "lstm_fwd_step: h_prev / fwd_pack not 16-byte aligned");
  const dim3 grid(hidden / LS_HB);
  if (dtype == OTR_F32)
    hipLaunchKernelGGL(lstm_fwd_step_kernel<float>, grid, dim3(LS_NT), 0, (hipStream_t)stream, gx, bias, (const float*)h_prev, c_prev,
                       (const uint4*)fwd_pack, h, (bf16_t*)h_bf16, c, act, (int)rows, hidden);
  else
    hipLaunchKernelGGL(lstm_fwd_step_kernel<bf16_t>, grid, dim3(LS_NT), 0, (hipStream_t)stream, gx, bias, (const bf16_t*)h_prev, c_prev,
                       (const uint4*)fwd_pack, h, (bf16_t*)h_bf16, c, act, (int)rows, hidden);
  return otr_check_launch("lstm_fwd_step");
}

extern "C" int32_t otr_lstm_bwd_step(const float* dy, const void* dg_next, const void* bwd_pack, const float* act, const float* c,
                                     const float* c_prev, const float* dc_in, float* dc_out, void* dg, int32_t dtype, int64_t rows,
                                     int32_t hidden, void* stream) {
  OTR_REQUIRE(dy && bwd_pack && act && c && dc_out && dg, "lstm_bwd_step: null pointer");
  OTR_REQUIRE(dtype == OTR_F32 || dtype == OTR_H16, "lstm_bwd_step: dtype must be OTR_F32 or this build's 16-bit type");
  OTR_REQUIRE(ls_fused_shape(rows, hidden), "lstm_bwd_step: rows %lld / hidden %d outside the limits", (long long)rows, hidden);
  OTR_REQUIRE(((uintptr_t)dg_next & 15) == 0 && ((uintptr_t)bwd_pack & 15) == 0, "lstm_bwd_step: dg_next / bwd_pack not 16-byte aligned");
  const dim3 grid(hidden / LS_HB);
  if (dtype == OTR_F32)
    hipLaunchKernelGGL(lstm_bwd_step_kernel<float>, grid, dim3(LS_NT), 0, (hipStream_t)stream, dy, (const float*)dg_next,
                       (const uint4*)bwd_pack, act, c, c_prev, dc_in, dc_out, (float*)dg, (int)rows, hidden);
  else
    hipLaunchKernelGGL(lstm_bwd_step_kernel<bf16_t>, grid, dim3(LS_NT), 0, (hipStream_t)stream, dy, (const bf16_t*)dg_next,
                       (const uint4*)bwd_pack, act, c, c_prev, dc_in, dc_out, (bf16_t*)dg, (int)rows, hidden);
  return otr_check_launch("lstm_bwd_step");
}

extern "C" int32_t otr_lstm_cell_fwd(const float* gx, const float* gh, const float* bias, const float* c_prev, float* h, void* h_bf16,
                                     float* c, float* act, int64_t rows, int32_t hidden, void* stream) {
  OTR_REQUIRE(gx && h && c && act, "lstm_cell_fwd: null pointer");
  OTR_REQUIRE(rows >= 0 && hidden > 0, "lstm_cell_fwd: bad shape");
  if (rows == 0) return 0;
  const int64_t n = rows * hidden, g = (n + 255) / 256;
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, (hipStream_t)stream, gx, gh, bias, c_prev,
                     h, (bf16_t*)h_bf16, c, act, rows, hidden);
  return otr_check_launch("lstm_cell_fwd");
}

extern "C" int32_t otr_lstm_cell_bwd(const float* dy, const float* dh_rec, const float* act, const float* c, const float* c_prev,
                                     const float* dc_in, float* dc_out, void* dg, int32_t dtype, int64_t rows, int32_t hidden, void* stream) {
  OTR_REQUIRE(dy && act && c && dc_out && dg, "lstm_cell_bwd: null pointer");
  OTR_REQUIRE(dtype == OTR_F32 || dtype == OTR_H16, "lstm_cell_bwd: dtype must be OTR_F32 or this build's 16-bit type");
  OTR_REQUIRE(rows >= 0 && hidden > 0, "lstm_cell_bwd: bad shape");
  if (rows == 0) return 0;
  const int64_t n = rows * hidden, g = (n + 255) / 256;
  const dim3 grid((unsigned)(g > 4096 ? 4096 : g));
  if (dtype == OTR_F32)
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, dy, dh_rec, act, c, c_prev, dc_in, dc_out,
                       (float*)dg, rows, hidden);
  else
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, dy, dh_rec, act, c, c_prev, dc_in, dc_out,
                       (bf16_t*)dg, rows, hidden);
  return otr_check_launch("lstm_cell_bwd");
}
