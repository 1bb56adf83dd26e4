// MixSpeech (otrans/train/trainer.py:155-201): utterances 2p and 2p + 1 of a padded batch mixed frame by frame with one weight per
// batch, out[p] = lam * x[2p] + (1 - lam) * x[2p + 1], with the length and mask of the longer of the two.  include/otrans_hip.h states
// the semantics.
//  * one launch: workgroup (chunk, p) owns MX_CHUNK = 4096 consecutive elements of the pair's row of T * F floats, a thread four quads
//    of four.  It writes every cell of its chunk of out[p] once, and the mask of the frames that START in the chunk.
//  * a frame at or past an input utterance's length counts as zero and is not read; cells at or past the pair's length are written as
//    zero without forming the expression.
//  * the arithmetic is the float32 composition of the reference: om = 1 - lam rounded once, each product rounded, then the sum.  The
//    expression is compiled with contraction off (mx_mix), so no fused multiply-add replaces the two roundings.
//  * loads and stores are 16 bytes wide where the row's base allows (x[2p], x[2p + 1] and out[p] judged separately), scalar otherwise;
//    lam is read from device memory by every thread (one cached line).
#include "common.h"

constexpr int MX_THREADS = 256;
constexpr int MX_QUADS = 4;                                   // quads of 4 floats per thread
constexpr int MX_CHUNK = MX_THREADS * 4 * MX_QUADS;           // elements per workgroup
constexpr int MX_MAX_P = 65535;                               // gridDim.y

__device__ __forceinline__ float mx_mix(float lam, float om, float a, float b) {
#pragma clang fp contract(off)
  const float pa = lam * a;
  const float pb = om * b;
  return pa + pb;
}

__device__ __forceinline__ int mx_live_frames(const int32_t* lengths, int b, int T) {
  const int len = lengths[b];
  return len < 0 ? 0 : (len > T ? T : len);
}

// v[0..3] = row[e .. e + 3], zero at and past n (never read there)
__device__ __forceinline__ void mx_load4(const float* row, bool vec, int64_t e, int64_t n, float v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (e >= n) return;
  if (vec && e + 4 <= n) {
    const uint4 u = ld_global_b128(row + e);
    v[0] = __uint_as_float(u.x); v[1] = __uint_as_float(u.y); v[2] = __uint_as_float(u.z); v[3] = __uint_as_float(u.w);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e + k < n) v[k] = row[e + k];
  }
}

__global__ __launch_bounds__(MX_THREADS) void mixspeech_mix_kernel(const float* x, int64_t pitch, const int32_t* lengths,
                                                                   const float* lam_p, int T, int F, float* out, int32_t* out_lengths,
                                                                   uint8_t* out_mask) {
  const int p = blockIdx.y, tid = threadIdx.x;
  const int la = mx_live_frames(lengths, 2 * p, T), lb = mx_live_frames(lengths, 2 * p + 1, T);
  const int len = la > lb ? la : lb;
  const int64_t TF = (int64_t)T * F, na = (int64_t)la * F, nb = (int64_t)lb * F, n = (int64_t)len * F;
  const int64_t e0 = (int64_t)blockIdx.x * MX_CHUNK;
  const int64_t e1 = e0 + MX_CHUNK < TF ? e0 + MX_CHUNK : TF;
  if (blockIdx.x == 0 && tid == 0) out_lengths[p] = len;
  {                                                           // the frames whose first element lies in [e0, e1)
    const int t1 = (int)((e1 + F - 1) / F);
    for (int t = (int)((e0 + F - 1) / F) + tid; t < t1; t += MX_THREADS) out_mask[(int64_t)p * T + t] = t < len ? 1 : 0;
  }
  const float lam = *lam_p;
  const float om = 1.f - lam;
  const float* xa = x + (int64_t)(2 * p) * pitch;
  const float* xb = xa + pitch;
  float* y = out + (int64_t)p * TF;
  const bool avec = ((uintptr_t)xa & 15) == 0, bvec = ((uintptr_t)xb & 15) == 0, yvec = ((uintptr_t)y & 15) == 0;
#pragma unroll
  for (int q = 0; q < MX_QUADS; ++q) {
    const int64_t e = e0 + (int64_t)(q * MX_THREADS + tid) * 4;
    if (e >= TF) continue;
    float a[4], b[4], v[4];
    mx_load4(xa, avec, e, na, a);
    mx_load4(xb, bvec, e, nb, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (e + k < n) ? mx_mix(lam, om, a[k], b[k]) : 0.f;
    if (yvec && e + 4 <= TF) {
      st_global_b128(y + e, make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < TF) y[e + k] = v[k];
    }
  }
}

extern "C" int32_t otr_mixspeech_mix(const float* x, int64_t pitch, const int32_t* lengths, const float* lam, int32_t B, int32_t T,
                                     int32_t F, float* out, int32_t* out_lengths, uint8_t* out_mask, void* stream) {
  OTR_REQUIRE(B >= 2 && T >= 1 && F >= 1 && (int64_t)T * F < (1ll << 31) && B / 2 <= MX_MAX_P,
              "mixspeech_mix: bad shape B=%d T=%d F=%d (B >= 2, B / 2 <= %d, T >= 1, F >= 1, T * F < 2^31)", B, T, F, MX_MAX_P);
  OTR_REQUIRE(x && lengths && lam && out && out_lengths && out_mask, "mixspeech_mix: null pointer");
  OTR_REQUIRE(pitch >= (int64_t)T * F, "mixspeech_mix: utterance pitch %lld below T * F = %lld", (long long)pitch, (long long)T * F);
  const int P = B / 2;                                        // an odd last utterance takes no part (trainer.py:160)
  const unsigned nchunk = (unsigned)(((int64_t)T * F + MX_CHUNK - 1) / MX_CHUNK);
  hipLaunchKernelGGL(mixspeech_mix_kernel, dim3(nchunk, (unsigned)P), dim3(MX_THREADS), 0, (hipStream_t)stream, x, pitch, lengths, lam, T,
                     F, out, out_lengths, out_mask);
  return otr_check_launch("mixspeech_mix");
}
