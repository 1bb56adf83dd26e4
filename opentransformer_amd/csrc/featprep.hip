// Feature preparation for device batch assembly: the reference's per-utterance chain after the fbank (otrans/data/audio.py:125-136:
// normalisation -> gaussian noise -> SpecAugment) applied while the packed ragged upload [sum T, F] is spread into the padded batch
// [B, Tmax, F], and the sums a global CMVN is formed from.  fp32 / fp64 only, identical in both builds; include/otrans_hip.h states
// the semantics.
//  * utterance b is n_b = lengths[b] * F contiguous floats; both kernels of otr_feature_prepare cut it (and its padded row of Tmax * F
//    floats) into chunks of FP_CHUNK = 4096 elements, one workgroup per chunk, a thread owning four quads of four consecutive elements.
//  * utterance normalisation (mode 1), first launch: a workgroup sums d = x - pivot and d * d of its chunk in fp64 (pivot = the
//    utterance's first value: with it the one-pass variance of data far from zero loses nothing to cancellation), lanes by a butterfly,
//    waves in index order, and writes the pair to the workspace.  Chunks past n_b write nothing.
//  * second launch (the only one in modes 0 and 2): every workgroup adds the utterance's partials in index order -- a wave-uniform loop,
//    so each workgroup forms the same bits -- rounds mean and std to fp32 as torch.std_mean does, and writes its chunk of dst:
//    (x - mean) / std + noise[b, f], zero inside a rectangle, zero at and past row lengths[b].  Every cell of dst is written once, by the
//    thread that read it, so the in-place padded form (src == dst, row_off[b] == b * Tmax) has no hazard: the pivot and the sums come
//    from the workspace, never from src again.  The workgroup also writes mask for the rows that START in its chunk.
//  * no floating-point atomics anywhere: the same call gives the same bits.
#include "common.h"

constexpr int FP_THREADS = 256;
constexpr int FP_QUADS = 4;                                   // quads of 4 floats per thread
constexpr int FP_CHUNK = FP_THREADS * 4 * FP_QUADS;           // elements per workgroup
constexpr int FP_MAX_NR = 64;
constexpr int FP_MAX_B = 65535;                               // gridDim.y

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int fp_live_frames(const int32_t* lengths, int b, int Tmax) {
  const int len = lengths[b];
  return len < 0 ? 0 : (len > Tmax ? Tmax : len);
}

// workspace: per utterance 1 + 2 * nchunk doubles = {pivot, (sum d, sum d*d) per chunk}
__global__ __launch_bounds__(FP_THREADS) void featprep_stats_kernel(const float* src, const int64_t* row_off, const int32_t* lengths,
                                                                    int Tmax, int F, int nchunk, double* ws) {
  __shared__ double s_part[FP_THREADS / 64][2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = (int64_t)fp_live_frames(lengths, b, Tmax) * F;
  const int64_t e0 = (int64_t)blockIdx.x * FP_CHUNK;
  if (e0 >= n) return;                                        // workgroup-uniform
  const float* x = src + row_off[b] * F;
  const bool vec = ((uintptr_t)x & 15) == 0;
  const double pivot = (double)x[0];
  double s = 0.0, ss = 0.0;
#pragma unroll
  for (int q = 0; q < FP_QUADS; ++q) {
    const int64_t e = e0 + (int64_t)(q * FP_THREADS + tid) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int live = 0;
    if (vec && e + 4 <= n) {
      const uint4 u = ld_global_b128(x + e);
      v[0] = __uint_as_float(u.x); v[1] = __uint_as_float(u.y); v[2] = __uint_as_float(u.z); v[3] = __uint_as_float(u.w);
      live = 4;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) { v[k] = x[e + k]; live = k + 1; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < live) {
        const double d = (double)v[k] - pivot;
        s += d;
        ss += d * d;
      }
  }
  s = wave_sum_f64(s);
  ss = wave_sum_f64(ss);
  if ((tid & 63) == 0) { s_part[tid >> 6][0] = s; s_part[tid >> 6][1] = ss; }
  __syncthreads();
  if (tid == 0) {
    double* w = ws + (int64_t)b * (1 + 2 * (int64_t)nchunk);
    double a = s_part[0][0], c = s_part[0][1];
#pragma unroll
    for (int i = 1; i < FP_THREADS / 64; ++i) { a += s_part[i][0]; c += s_part[i][1]; }
    w[1 + 2 * (int64_t)blockIdx.x] = a;
    w[2 + 2 * (int64_t)blockIdx.x] = c;
    if (blockIdx.x == 0) w[0] = pivot;
  }
}

template <int MODE>
__global__ __launch_bounds__(FP_THREADS) void featprep_apply_kernel(const float* src, const int64_t* row_off, const int32_t* lengths,
                                                                    int Tmax, int F, FastDiv fd, const float* gmean, const float* gstd,
                                                                    const float* noise, const int32_t* ranges, int NR, float* dst,
                                                                    uint8_t* mask, float* stats, const double* ws, int nchunk) {
  __shared__ int s_r[FP_MAX_NR * 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = fp_live_frames(lengths, b, Tmax);
  const int64_t n = (int64_t)len * F, TF = (int64_t)Tmax * F;
  const int64_t e0 = (int64_t)blockIdx.x * FP_CHUNK;
  const int64_t e1 = e0 + FP_CHUNK < TF ? e0 + FP_CHUNK : TF;
  if (NR > 0) {
    if (tid < NR * 4) s_r[tid] = ranges[(int64_t)b * NR * 4 + tid];
    __syncthreads();
  }
  if (mask) {                                                 // the rows whose first element lies in [e0, e1)
    const int t1 = (int)((e1 + F - 1) / F);
    for (int t = (int)((e0 + F - 1) / F) + tid; t < t1; t += FP_THREADS) mask[(int64_t)b * Tmax + t] = t < len ? 1 : 0;
  }
  float mean = 0.f, sd = 1.f;
  if (MODE == 1 && n > 0) {                                   // wave-uniform: the same additions in the same order in every workgroup
    const double* w = ws + (int64_t)b * (1 + 2 * (int64_t)nchunk);
    const int live_chunks = (int)((n + FP_CHUNK - 1) / FP_CHUNK);
    double S = 0.0, SS = 0.0;
    for (int c = 0; c < live_chunks; ++c) { S += w[1 + 2 * c]; SS += w[2 + 2 * c]; }
    const double dn = (double)n;
    double var = (SS - S * S / dn) / (dn - 1.0);              // unbiased; n == 1 gives 0 / 0 as torch.std_mean does
    if (var < 0.0) var = 0.0;                                 // rounding of a (near-)constant utterance; keeps a NaN
    mean = (float)(w[0] + S / dn);
    sd = (float)sqrt(var);
    if (stats && blockIdx.x == 0 && tid == 0) { stats[2 * b] = mean; stats[2 * b + 1] = sd; }
  }
  const float* x = src + (n > 0 ? row_off[b] * F : 0);        // an empty utterance's offset is never used
  float* y = dst + (int64_t)b * TF;
  const bool svec = ((uintptr_t)x & 15) == 0, dvec = ((uintptr_t)y & 15) == 0;
  const float* nz = noise ? noise + (int64_t)b * F : nullptr;
#pragma unroll
  for (int q = 0; q < FP_QUADS; ++q) {
    const int64_t e = e0 + (int64_t)(q * FP_THREADS + tid) * 4;
    if (e >= TF) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < n) {
      if (svec && e + 4 <= n) {
        const uint4 u = ld_global_b128(x + e);
        v[0] = __uint_as_float(u.x); v[1] = __uint_as_float(u.y); v[2] = __uint_as_float(u.z); v[3] = __uint_as_float(u.w);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < n) v[k] = x[e + k];
      }
      int t = (int)fdiv((uint32_t)e, fd);
      int f = (int)(e - (int64_t)t * F);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e + k < n) {
          float r = v[k];
          if (MODE == 1) r = (r - mean) / sd;
          if (MODE == 2) r = (r - gmean[f]) / gstd[f];
          if (nz) r += nz[f];
          for (int i = 0; i < NR; ++i)
            if (t >= s_r[4 * i] && t < s_r[4 * i + 1] && f >= s_r[4 * i + 2] && f < s_r[4 * i + 3]) r = 0.f;
          v[k] = r;
        } else {
          v[k] = 0.f;
        }
        if (++f == F) { f = 0; ++t; }
      }
    }
    if (dvec && e + 4 <= TF) {
      st_global_b128(y + e, make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < TF) y[e + k] = v[k];
    }
  }
}

// ---------------------------------------------------------------- sums for a global CMVN
// One workgroup owns CM_DIMS feature dimensions and is the only writer of their entries of acc: thread (slot, d) adds frames slot,
// slot + 64, ... of every utterance in batch order in fp64, the 64 slots are added in index order, and the total goes onto acc with a
// plain read-modify-write (calls on one stream are ordered).  A quarter wave reads 64 contiguous bytes of a frame.
constexpr int CM_DIMS = 16, CM_SLOTS = 64;

__global__ __launch_bounds__(CM_DIMS * CM_SLOTS) void cmvn_accumulate_kernel(const float* src, const int64_t* row_off,
                                                                             const int32_t* lengths, int B, int F, double* acc) {
  __shared__ double s_sum[CM_SLOTS][CM_DIMS], s_sq[CM_SLOTS][CM_DIMS];
  const int d = threadIdx.x % CM_DIMS, slot = threadIdx.x / CM_DIMS;
  const int f = blockIdx.x * CM_DIMS + d;
  double s = 0.0, ss = 0.0;
  if (f < F) {
    for (int b = 0; b < B; ++b) {
      const int len = lengths[b];
      if (len <= 0) continue;
      const float* x = src + row_off[b] * F + f;
      for (int t = slot; t < len; t += CM_SLOTS) {
        const double v = (double)x[(int64_t)t * F];
        s += v;
        ss += v * v;
      }
    }
  }
  s_sum[slot][d] = s;
  s_sq[slot][d] = ss;
  __syncthreads();
  if (slot == 0 && f < F) {
    double a = s_sum[0][d], c = s_sq[0][d];
    for (int i = 1; i < CM_SLOTS; ++i) { a += s_sum[i][d]; c += s_sq[i][d]; }
    acc[f] += a;
    acc[F + f] += c;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t frames = 0;
    for (int b = 0; b < B; ++b) frames += lengths[b] > 0 ? lengths[b] : 0;
    acc[2 * (int64_t)F] += (double)frames;
  }
}

// ---------------------------------------------------------------- entries
static bool featprep_shape_ok(int64_t B, int64_t Tmax, int64_t F) {
  return B >= 0 && B <= FP_MAX_B && Tmax > 0 && F > 0 && Tmax * F < (1ll << 31);
}
static int64_t featprep_chunks(int64_t Tmax, int64_t F) { return (Tmax * F + FP_CHUNK - 1) / FP_CHUNK; }

extern "C" int64_t otr_feature_prepare_workspace_bytes(int32_t B, int32_t Tmax, int32_t F) {
  if (!featprep_shape_ok(B, Tmax, F)) return -1;
  return (int64_t)B * (1 + 2 * featprep_chunks(Tmax, F)) * (int64_t)sizeof(double);
}

extern "C" int32_t otr_feature_prepare(const float* src, const int64_t* row_off, const int32_t* lengths, int32_t B, int32_t Tmax,
                                       int32_t F, int32_t norm_mode, const float* gmean, const float* gstd, const float* noise,
                                       const int32_t* ranges, int32_t NR, float* dst, uint8_t* mask, float* stats, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  OTR_REQUIRE(featprep_shape_ok(B, Tmax, F), "feature_prepare: bad shape B=%d Tmax=%d F=%d (0 <= B <= %d, Tmax * F < 2^31)", B, Tmax, F,
              FP_MAX_B);
  OTR_REQUIRE(src && row_off && lengths && dst, "feature_prepare: null pointer");
  OTR_REQUIRE(NR >= 0 && NR <= FP_MAX_NR && (NR == 0 || ranges), "feature_prepare: NR=%d rectangles, 0 .. %d supported, with ranges", NR,
              FP_MAX_NR);
  OTR_REQUIRE(norm_mode >= 0 && norm_mode <= 2, "feature_prepare: norm_mode=%d must be 0 (copy), 1 (utterance) or 2 (global)", norm_mode);
  OTR_REQUIRE(norm_mode != 2 || (gmean && gstd), "feature_prepare: norm_mode 2 needs gmean and gstd");
  const int64_t need = otr_feature_prepare_workspace_bytes(B, Tmax, F);
  OTR_REQUIRE(workspace_bytes >= need && (workspace || need == 0) && ((uintptr_t)workspace & 7) == 0,
              "feature_prepare: workspace of %lld bytes, %lld needed, 8-byte aligned", (long long)workspace_bytes, (long long)need);
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int nchunk = (int)featprep_chunks(Tmax, F);
  const dim3 grid((unsigned)nchunk, (unsigned)B), block(FP_THREADS);
  const FastDiv fd = make_fastdiv((uint32_t)F);
  double* ws = (double*)workspace;
  if (!ranges) NR = 0;
  if (norm_mode == 1) {
    hipLaunchKernelGGL(featprep_stats_kernel, grid, block, 0, s, src, row_off, lengths, Tmax, F, nchunk, ws);
    hipLaunchKernelGGL(featprep_apply_kernel<1>, grid, block, 0, s, src, row_off, lengths, Tmax, F, fd, gmean, gstd, noise, ranges, NR, dst,
                       mask, stats, (const double*)ws, nchunk);
  } else if (norm_mode == 2) {
    hipLaunchKernelGGL(featprep_apply_kernel<2>, grid, block, 0, s, src, row_off, lengths, Tmax, F, fd, gmean, gstd, noise, ranges, NR, dst,
                       mask, stats, (const double*)ws, nchunk);
  } else {
    hipLaunchKernelGGL(featprep_apply_kernel<0>, grid, block, 0, s, src, row_off, lengths, Tmax, F, fd, gmean, gstd, noise, ranges, NR, dst,
                       mask, stats, (const double*)ws, nchunk);
  }
  return otr_check_launch("feature_prepare");
}

extern "C" int32_t otr_cmvn_accumulate(const float* src, const int64_t* row_off, const int32_t* lengths, int32_t B, int32_t F, double* acc,
                                       void* stream) {
  OTR_REQUIRE(B >= 0 && F > 0, "cmvn_accumulate: bad shape B=%d F=%d", B, F);
  OTR_REQUIRE(src && row_off && lengths && acc, "cmvn_accumulate: null pointer");
  OTR_REQUIRE(((uintptr_t)acc & 7) == 0, "cmvn_accumulate: acc must be 8-byte aligned");
  if (B == 0) return 0;
  hipLaunchKernelGGL(cmvn_accumulate_kernel, dim3((unsigned)((F + CM_DIMS - 1) / CM_DIMS)), dim3(CM_DIMS * CM_SLOTS), 0,
                     (hipStream_t)stream, src, row_off, lengths, B, F, acc);
  return otr_check_launch("cmvn_accumulate");
}
