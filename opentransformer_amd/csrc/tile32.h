// Device helpers for 32 x 32 MFMA tiles (v_mfma_f32_32x32x16 on the 16-bit type, mma32 in common.h) shared by the row-block,
// fused-FFN, decoder-layer and encoder-attention kernels: the accumulator and operand-fragment conventions, the fragment reads of
// the LDS images they stage, the accumulator-tile -> operand-fragment / row-major / column-sum conversions, and the GLU's sigmoid.
//
// Accumulator tile: lane (m = lane & 31, hi = lane >> 5) holds columns 8q + 4hi + (r & 3), q = r >> 2, of row m in its 16 registers.
// Operand fragment (uint4): lane (m, hi) holds contraction elements 16 ks + 8 hi .. + 7 of row m for contraction step ks.
#pragma once
#include "common.h"

constexpr int FF_RB = 32;   // rows of one MFMA B-operand tile (= rows per workgroup of the v1 kernels)

__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// 32 rows x D 16-bit activations -> LDS as 16-byte chunks, chunk index XOR (row & 15): the B-operand read of lane
// (m = lane&31, hi) -- chunk (2*ks + hi) of row m -- is then bank-conflict free for ds_read_b128
template <int D, int NTHR = 256>
__device__ __forceinline__ void stage_rows(uint4* dst, const uint16_t* src, int row0, int M, int tid) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int i = tid; i < FF_RB * CPR; i += NTHR) {
    const int r = i / CPR, ch = i % CPR;
    const int gr = min(row0 + r, M - 1);
    dst[r * CPR + (ch ^ (r & 15))] = ld_global_b128(src + (int64_t)gr * D + ch * 8);
  }
}
// fragment (m, hi, ks) of such rows (D 16-bit elements each)
template <int D> __device__ __forceinline__ uint4 frag_xor(const uint4* rows, int m, int hi, int ks) {
  return rows[m * (D / 8) + ((2 * ks + hi) ^ (m & 15))];
}
// fragment (m, hi, ks) of a padded row-major LDS image, `stride` bytes per row
__device__ __forceinline__ uint4 frag_rm(const unsigned char* img, int stride, int m, int hi, int ks) {
  return *reinterpret_cast<const uint4*>(img + m * stride + (2 * ks + hi) * 16);
}
// fragment of a transposed LDS image (`stride` bytes per row) with the contraction slots of step k2 in ACCUMULATOR order: elements
// col0 + 16 k2 + 4 hi + e, then + 8 (e < 4) of row `row` -- so that an accumulator tile converted by frag_pack8 is the other operand
__device__ __forceinline__ uint4 frag_tr(const unsigned char* timg, int stride, int row, int col0, int hi, int k2) {
  const unsigned char* vr = timg + row * stride + (col0 + 16 * k2 + 4 * hi) * 2;
  const uint2 lo = *reinterpret_cast<const uint2*>(vr), up = *reinterpret_cast<const uint2*>(vr + 16);
  return make_uint4(lo.x, lo.y, up.x, up.y);
}

__device__ __forceinline__ void tile_zero(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
template <int N> __device__ __forceinline__ void tile_zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// eight floats -> one operand fragment of the 16-bit type
__device__ __forceinline__ uint4 frag_pack8(const float* v) {
  return make_uint4(pack2h(v[0], v[1]), pack2h(v[2], v[3]), pack2h(v[4], v[5]), pack2h(v[6], v[7]));
}

// accumulator tile (16 floats: hidden units 8q + 4hi + (r&3), q = r>>2, of row m = lane&31) -> two B-operand fragments
__device__ __forceinline__ void tile_to_frags(const float* v, uint4& f0, uint4& f1) {
  f0 = frag_pack8(v);
  f1 = frag_pack8(v + 8);
}

// accumulator tile -> red[m][col0 + 8q + 4hi + (r&3)] (row stride RS floats)
template <int RS> __device__ __forceinline__ void put_tile(float* red, const f32x16& a, int col0, int lane) {
  const int m = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(red + m * RS + col0 + 8 * q + 4 * hi) = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
}

// store an accumulator tile as 32 consecutive 16-bit elements of row m (row-major consumer: the weight-gradient GEMM).
// The row's 64 bytes are split over lanes m and m+32 in 8-byte pieces; one v_permlane32_swap per dword turns them into
// 16-byte pieces (cdna_hip_programming.md T21): lane (m, hi) then owns elements [8(q0+hi), 8(q0+hi)+8) for q0 = 0, 2.
__device__ __forceinline__ void store_tile_row(uint16_t* rowp, const uint4& f0, const uint4& f1, int hi, bool live) {
  uint32_t w[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
  for (int q0 = 0; q0 < 4; q0 += 2) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      auto r = __builtin_amdgcn_permlane32_swap(w[2 * q0 + e], w[2 * q0 + 2 + e], false, false);
      w[2 * q0 + e] = r[0];
      w[2 * q0 + 2 + e] = r[1];
    }
    if (live) st_global_b128(rowp + 8 * (q0 + hi), make_uint4(w[2 * q0], w[2 * q0 + 1], w[2 * q0 + 2], w[2 * q0 + 3]));
  }
}

// column sums of an accumulator tile over its 32 rows: the 16 registers of lane (m, hi) are hidden units 8q + 4hi + (r&3) of
// row m.  Reduce-scatter butterfly over the 32 lanes of a half-wave (xor 16, 8, 4, 2 halve the register set each step, xor 1
// finishes): 16 shuffles per tile instead of 80 for sixteen independent butterflies; lane m ends up with the total of
// register r = (m4 m3 m2 m1) and the even lanes store it.  dst = the 32 floats of this tile in the partial-sum row.
__device__ __forceinline__ void tile_colsum_store(const float* v, float* dst, int lane, int hi, bool rows_live) {
  const int m = lane & 31;
  const bool b4 = m & 16, b3 = m & 8, b2 = m & 4, b1 = m & 2;
  float a[8], b[4], c[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float lo = rows_live ? v[i] : 0.f, hi_ = rows_live ? v[8 + i] : 0.f;
    a[i] = (b4 ? hi_ : lo) + __shfl_xor(b4 ? lo : hi_, 16);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = (b3 ? a[4 + i] : a[i]) + __shfl_xor(b3 ? a[i] : a[4 + i], 8);
#pragma unroll
  for (int i = 0; i < 2; ++i) c[i] = (b2 ? b[2 + i] : b[i]) + __shfl_xor(b2 ? b[i] : b[2 + i], 4);
  float d = (b1 ? c[1] : c[0]) + __shfl_xor(b1 ? c[0] : c[1], 2);
  d += __shfl_xor(d, 1);
  const int r = ((m >> 4) & 1) * 8 + ((m >> 3) & 1) * 4 + ((m >> 2) & 1) * 2 + ((m >> 1) & 1);
  if ((m & 1) == 0) dst[8 * (r >> 2) + 4 * hi + (r & 3)] = d;
}
