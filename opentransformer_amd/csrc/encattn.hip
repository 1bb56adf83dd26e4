// Encoder self-attention backward for the shipped shape class (module/attention.py:23-46 under autograd; encoder/transformer.py:47-49):
// 16-bit operands, head dim 64, no causal mask, no score bias, T <= 512 frames after the frontend (AISHELL's 10 s bench utterances: 249; its longest,
// ~14.5 s: 363).  Up to 256 frames one (utterance, head) lives in LDS whole (below); beyond (r06, MULTI) the SAME code walks the streamed side in
// super-chunks of 256 rows, restaging the images between them, and the owned side is cut into blocks of 256 rows, one workgroup each.
//
// Why a second kernel beside attention.hip: that one is generic (any T, head dim, fp32) -- 16-row MFMA tiles, the streamed side
// re-staged block by block behind two barriers each, every 16-cycle MFMA fed by a fresh 1 KiB LDS operand.  At 32 x 4 x 249 x 64 it
// took 34 us for 7 GFLOP (LDS-read and barrier bound: ~770 KiB of operand reads per CU and block step against 128 B/clk).
// Here one (utterance, head) is small enough to live in LDS WHOLE:
//   * 2 workgroups per (utterance, head) -- one per ORIENTATION, 8 waves each, 256 workgroups for 32 x 4: one per CU, the pair on
//     one XCD (they read the same rows);
//       orientation 0: lane = query, registers = keys   -> dQ       (wave w owns queries 32 w .. + 31)
//       orientation 1: lane = key,   registers = queries -> dK, dV  (wave w owns keys 32 w .. + 31)
//   * the streamed side is staged ONCE (row-major image for the products contracted over the head dim, transposed image for the ones
//     contracted over the streamed index), then every wave walks the 32-row tiles on its own: no barrier, no global load in the loop;
//   * 32 x 32 x 16 MFMAs: half the operand bytes per flop of the 16-row tiles; the owned side's fragments stay in registers;
//   * P and dS go from the accumulators straight back into MFMA operands (the accumulator layout is an operand layout once the
//     contraction slots are taken in accumulator order -- the transposed images are read in that order, frag_tr in tile32.h);
//   * delta = rowsum(dO . O) is formed on the way in (no separate pass), outputs leave through LDS as whole 128-byte rows.
// Work per (utterance, head): 7 products of T x T x 64 (S and dP are formed in both orientations) -- the same recompute as before.
#include "tile32.h"

namespace {

constexpr int EA_T = 256;                 // rows of one LDS image: most frames served in ONE pass
constexpr int EA_TMAX = 512;              // most frames served at all (own blocks x streamed super-chunks of EA_T)
constexpr int EA_DK = 64;
constexpr int EA_HS = EA_DK * 2 + 16;     // bytes per row of a row-major [T][64] 16-bit image
constexpr int EA_TS = EA_T * 2 + 8;       // bytes per row of a transposed [64][T] 16-bit image
constexpr int EA_RM = EA_T * EA_HS;       // 36864
constexpr int EA_TR = EA_DK * EA_TS;      // 33280
constexpr float EA_LOG2E = 1.4426950408889634f;

struct EaArgs {
  unsigned long long* trace;
  const uint16_t *q, *k, *v, *o, *do_;
  uint16_t *dq, *dk, *dv;
  const uint8_t* key_mask;
  const float* lse;
  int B, H, T;
  int64_t q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts;
  float scale;
};


// The streamed side is staged in CHUNKS of 64 rows (two tiles): the workgroup issues every global load of its set-up at once, chunk by
// chunk (vmcnt retires in order), and starts on the tiles of chunk c while chunks c+1.. are still travelling -- the set-up is bound by
// the CU's ingest (~160 KiB per workgroup, ~10 k cycles when it was waited for in one piece, a third of the launch).
// piece (row 64 c + tid / 8, 16 bytes tid % 8) of chunk c of a [T][64] matrix (row stride ts elements); rows past T are clamped here and
// zeroed when they are written
__device__ __forceinline__ uint4 ea_issue(const uint16_t* src, int64_t ts, int T, int tid, int c) {
  const int row = 64 * c + (tid >> 3);
  return ld_global_b128(src + (int64_t)min(row, T - 1) * ts + 8 * (tid & 7));
}
// -> row-major image.  DOT: w is the same piece of a second matrix and sdot[row] = sum_d a[row][d] b[row][d] is left in LDS.
template <bool DOT>
__device__ __forceinline__ void ea_stage_rm(unsigned char* img, uint4 q, uint4 w, float* sdot, int T, int tid, int c) {
  const int row = 64 * c + (tid >> 3), ch = tid & 7;
  const uint32_t live = (uint32_t)0 - (uint32_t)(row < T);
  q.x &= live; q.y &= live; q.z &= live; q.w &= live;
  *reinterpret_cast<uint4*>(img + row * EA_HS + ch * 16) = q;
  if constexpr (DOT) {
    const uint32_t a[4] = {q.x, q.y, q.z, q.w}, b[4] = {w.x, w.y, w.z, w.w};
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) part += h2f_lo(a[e]) * h2f_lo(b[e]) + h2f_hi(a[e]) * h2f_hi(b[e]);
    part += __shfl_xor(part, 1);
    part += __shfl_xor(part, 2);
    part += __shfl_xor(part, 4);
    if (ch == 0) sdot[row] = part;
  }
}
// transposed image of chunk c of a staged row-major image: timg[d][row], two rows per 32-bit store; thread t (0 .. 255) takes the row pair
// 32 c + t % 32 and the 16-byte piece t / 32, elements 2 e0 .. 2 e0 + 2 ne - 1 of it.  Call between two barriers.
__device__ __forceinline__ void ea_transpose(unsigned char* timg, const unsigned char* img, int c, int t, int e0, int ne) {
  const int rp = 32 * c + (t & 31), ch = (t >> 5) & 7;
  const uint4 a = *reinterpret_cast<const uint4*>(img + (2 * rp) * EA_HS + ch * 16);
  const uint4 b = *reinterpret_cast<const uint4*>(img + (2 * rp + 1) * EA_HS + ch * 16);
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < e0 || e >= e0 + ne) continue;
    *reinterpret_cast<uint32_t*>(timg + (8 * ch + 2 * e) * EA_TS + 4 * rp) = (aw[e] & 0xffffu) | (bw[e] << 16);
    *reinterpret_cast<uint32_t*>(timg + (8 * ch + 2 * e + 1) * EA_TS + 4 * rp) = (aw[e] >> 16) | (bw[e] & 0xffff0000u);
  }
}

// own side: the four contraction-step fragments of row `row` (lane (m, hi) holds elements 16 ks + 8 hi .. + 7)
__device__ __forceinline__ void ea_load_frags(uint4 (&f)[4], const uint16_t* src, int64_t ts, int row, int hi) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f[ks] = ld_global_b128(src + (int64_t)row * ts + 16 * ks + 8 * hi);
}

// accumulator tiles (lane = own row m, registers = head dim 32 ct + 8 q + 4 hi + (r & 3)) x scale -> this wave's 32 rows of a row-major
// image -> memory as whole 128-byte rows
// live = false: the lane's row is written as zeros (whatever the accumulators hold, NaN included)
__device__ __forceinline__ void ea_put_rows(const f32x16 (&acc)[2], float scale, bool live, unsigned char* og, int lane) {
  const int m = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint2 v = make_uint2(pack2h(acc[ct][4 * q] * scale, acc[ct][4 * q + 1] * scale), pack2h(acc[ct][4 * q + 2] * scale, acc[ct][4 * q + 3] * scale));
      if (!live) v = make_uint2(0u, 0u);
      *reinterpret_cast<uint2*>(og + m * EA_HS + (32 * ct + 8 * q + 4 * hi) * 2) = v;
    }
}
__device__ __forceinline__ void ea_store_rows(const f32x16 (&acc)[2], float scale, bool live, unsigned char* og, uint16_t* dst, int64_t ts, int row0,
                                              int T, int lane) {
  ea_put_rows(acc, scale, live, og, lane);
  wait_lds();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = 8 * q + (lane >> 3), ch = lane & 7;
    if (row0 + j < T) st_global_b128(dst + (int64_t)(row0 + j) * ts + 8 * ch, *reinterpret_cast<const uint4*>(og + j * EA_HS + ch * 16));
  }
  wait_lds();
}

constexpr int EA_SMEM = 2 * EA_RM + 2 * EA_TR + 2 * EA_T * 4;

// MULTI = false: T <= 256, one own block, one super-chunk -- every `s0` / `o0` below folds to 0 and the code is the round-4 kernel.
// MULTI = true: own block ob = rows 256 ob .. (one workgroup per block, orientation and (utterance, head)), streamed super-chunks
// s0 = 0, 256, ...: the accumulators of the own rows live across them, the images are restaged behind a barrier.
template <bool MULTI>
__global__ __launch_bounds__(512, 1) void encattn_bwd_kernel(EaArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[EA_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, m = lane & 31, hi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the two orientations of one (utterance, head) get workgroup ids equal modulo 8: one XCD (placement observed, used for locality only)
  const int xcd = (int)blockIdx.x & 7, kk = (int)blockIdx.x >> 3;
  const int T = p.T;
  const int nob = MULTI ? (T + EA_T - 1) / EA_T : 1;               // own blocks
  const int orient = kk & 1, ob = MULTI ? (kk >> 1) % nob : 0, g = (MULTI ? (kk >> 1) / nob : (kk >> 1)) * 8 + xcd;
  if (g >= p.H * p.B) return;
  const int h = g % p.H, b = g / p.H;
  const int o0 = ob * EA_T;                                        // first own row of this workgroup
  const float sc2 = p.scale * EA_LOG2E;
  const uint16_t* Q = p.q + (int64_t)b * p.q_bs + h * EA_DK;
  const uint16_t* K = p.k + (int64_t)b * p.k_bs + h * EA_DK;
  const uint16_t* V = p.v + (int64_t)b * p.v_bs + h * EA_DK;
  const uint16_t* O = p.o + (int64_t)b * p.o_bs + h * EA_DK;
  const uint16_t* dO = p.do_ + (int64_t)b * p.o_bs + h * EA_DK;
  const float* lse = p.lse + ((int64_t)b * p.H + h) * T;
  const uint8_t* km = p.key_mask ? p.key_mask + (int64_t)b * T : nullptr;
  const int own = o0 + 32 * wid + m;                             // this lane's own row (query or key)
  const int ownc = min(own, T - 1);
  const bool wave_live = o0 + 32 * wid < T;                      // this wave owns at least one real row
  OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 0, g < 256);

  if (orient == 0) {
    // ------------------------------------------------------------------ lane = query: dQ = scale . dS K
    unsigned char* krm = smem;
    unsigned char* vrm = smem + EA_RM;
    unsigned char* kt = smem + 2 * EA_RM;
    float* kbias = reinterpret_cast<float*>(smem + 2 * EA_RM + EA_TR);          // 0 for a live key, -inf for a masked one / past T
    uint4 gk[4], gv[4], qf[4], dof[4], of[4];
    ea_load_frags(qf, Q, p.q_ts, ownc, hi);                                      // the own side first: the first tile needs it
    ea_load_frags(dof, dO, p.o_ts, ownc, hi);
    ea_load_frags(of, O, p.o_ts, ownc, hi);
    const float l0 = lse[ownc];
    uint8_t kmb = km ? km[min(tid, T - 1)] : (uint8_t)1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gk[c] = ea_issue(K, p.k_ts, T, tid, c);
      gv[c] = ea_issue(V, p.v_ts, T, tid, c);
    }
    __builtin_amdgcn_sched_barrier(0);
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 1, g < 256);
    float del = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const uint32_t a[4] = {dof[ks].x, dof[ks].y, dof[ks].z, dof[ks].w}, c[4] = {of[ks].x, of[ks].y, of[ks].z, of[ks].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) del += h2f_lo(a[e]) * h2f_lo(c[e]) + h2f_hi(a[e]) * h2f_hi(c[e]);
    }
    del += __shfl_xor(del, 32);
    // a query row with no live key at all (lse = -inf) has P = 0 everywhere; rows past T contribute nothing and are not stored
    const float nl = (own < T && l0 != -__builtin_huge_valf()) ? -l0 * EA_LOG2E : -__builtin_huge_valf();
    f32x16 dq[2];
    tile_zero(dq[0]); tile_zero(dq[1]);
    auto tile = [&](int jt) {
      const unsigned char* kr = krm + jt * 32 * EA_HS;
      const unsigned char* vr = vrm + jt * 32 * EA_HS;
      f32x16 st, dp;
      tile_zero(st); tile_zero(dp);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { mma32(st, frag_rm(kr, EA_HS, m, hi, ks), qf[ks]); mma32(dp, frag_rm(vr, EA_HS, m, hi, ks), dof[ks]); }
      float dsv[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 kb = *reinterpret_cast<const float4*>(kbias + jt * 32 + 8 * q + 4 * hi);
        const float kb4[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], sc2, nl) + kb4[e]);
          dsv[r] = pe * (dp[r] - del);
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const uint4 pb = frag_pack8(dsv + 8 * k2);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) mma32(dq[ct], frag_tr(kt, EA_TS, 32 * ct + m, jt * 32, hi, k2), pb);
      }
    };
    for (int s0 = 0; s0 < (MULTI ? T : 1); s0 += EA_T) {           // streamed super-chunks (one when T <= 256)
      const int Ts = MULTI ? min(EA_T, T - s0) : T, nt = (Ts + 31) >> 5;
      if (MULTI && s0 > 0) {
        __syncthreads();                                           // every wave is done with the previous super-chunk's images
        kmb = km ? km[min(s0 + tid, T - 1)] : (uint8_t)1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          gk[c] = ea_issue(K + (int64_t)s0 * p.k_ts, p.k_ts, Ts, tid, c);
          gv[c] = ea_issue(V + (int64_t)s0 * p.v_ts, p.v_ts, Ts, tid, c);
        }
      }
      if (tid < EA_T) kbias[tid] = (tid < Ts && kmb) ? 0.f : -__builtin_huge_valf();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (2 * c >= nt) break;                                     // uniform over the workgroup
        ea_stage_rm<false>(krm, gk[c], gk[c], nullptr, Ts, tid, c);
        ea_stage_rm<false>(vrm, gv[c], gv[c], nullptr, Ts, tid, c);
        __syncthreads();
        ea_transpose(kt, krm, c, tid & 255, 2 * (tid >> 8), 2);
        __syncthreads();
        if (c == 0) OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 2, g < 256);
        if (wave_live) {
          tile(2 * c);
          if (2 * c + 1 < nt) tile(2 * c + 1);
        }
      }
    }
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 3, g < 256);
    __syncthreads();                                               // every wave is done with the images: they become staging space
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 4, g < 256);
    if (wave_live) ea_store_rows(dq, p.scale, true, krm + 32 * wid * EA_HS, p.dq + (int64_t)b * p.q_bs + h * EA_DK, p.q_ts, o0 + 32 * wid, T, lane);
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 5, g < 256);
  } else {
    // ------------------------------------------------------------------ lane = key: dV = P^T dO, dK = scale . dS^T Q
    unsigned char* qrm = smem;
    unsigned char* dorm = smem + EA_RM;
    unsigned char* qt = smem + 2 * EA_RM;
    unsigned char* dot = smem + 2 * EA_RM + EA_TR;
    float* nls = reinterpret_cast<float*>(smem + 2 * EA_RM + 2 * EA_TR);       // -lse log2(e) per query (-inf: no live key / past T)
    float* dels = nls + EA_T;
    uint4 gq[4], gdo[4], go[4], kf[4], vf[4];
    ea_load_frags(kf, K, p.k_ts, ownc, hi);                                      // the own side first: the first tile needs it
    ea_load_frags(vf, V, p.v_ts, ownc, hi);
    float l0 = lse[min(tid, T - 1)];
    const uint8_t kmb = km ? km[ownc] : (uint8_t)1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gq[c] = ea_issue(Q, p.q_ts, T, tid, c);
      gdo[c] = ea_issue(dO, p.o_ts, T, tid, c);
      go[c] = ea_issue(O, p.o_ts, T, tid, c);
    }
    __builtin_amdgcn_sched_barrier(0);
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 1, g < 256);
    // a masked key (or one past T) only pollutes ITS OWN dk / dv rows -- the lane is a column of every product here -- so the loop
    // carries no mask at all and the rows are zeroed on their way out
    const bool keyok = own < T && kmb;
    f32x16 dk[2], dv[2];
    tile_zero(dk[0]); tile_zero(dk[1]); tile_zero(dv[0]); tile_zero(dv[1]);
    auto tile = [&](int it) {
      const unsigned char* qr = qrm + it * 32 * EA_HS;
      const unsigned char* dr = dorm + it * 32 * EA_HS;
      f32x16 st, dp;
      tile_zero(st); tile_zero(dp);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { mma32(st, frag_rm(qr, EA_HS, m, hi, ks), kf[ks]); mma32(dp, frag_rm(dr, EA_HS, m, hi, ks), vf[ks]); }
      float pv[16], dsv[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 nl = *reinterpret_cast<const float4*>(nls + it * 32 + 8 * q + 4 * hi);
        const float4 de = *reinterpret_cast<const float4*>(dels + it * 32 + 8 * q + 4 * hi);
        const float nl4[4] = {nl.x, nl.y, nl.z, nl.w}, de4[4] = {de.x, de.y, de.z, de.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          pv[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], sc2, nl4[e]));
          dsv[r] = pv[r] * (dp[r] - de4[e]);
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const uint4 pb = frag_pack8(pv + 8 * k2), sb = frag_pack8(dsv + 8 * k2);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          mma32(dv[ct], frag_tr(dot, EA_TS, 32 * ct + m, it * 32, hi, k2), pb);
          mma32(dk[ct], frag_tr(qt, EA_TS, 32 * ct + m, it * 32, hi, k2), sb);
        }
      }
    };
    for (int s0 = 0; s0 < (MULTI ? T : 1); s0 += EA_T) {           // streamed super-chunks of queries (one when T <= 256)
      const int Ts = MULTI ? min(EA_T, T - s0) : T, nt = (Ts + 31) >> 5;
      if (MULTI && s0 > 0) {
        __syncthreads();                                           // every wave is done with the previous super-chunk's images
        l0 = lse[min(s0 + tid, T - 1)];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          gq[c] = ea_issue(Q + (int64_t)s0 * p.q_ts, p.q_ts, Ts, tid, c);
          gdo[c] = ea_issue(dO + (int64_t)s0 * p.o_ts, p.o_ts, Ts, tid, c);
          go[c] = ea_issue(O + (int64_t)s0 * p.o_ts, p.o_ts, Ts, tid, c);
        }
      }
      if (tid < EA_T) nls[tid] = (tid < Ts && l0 != -__builtin_huge_valf()) ? -l0 * EA_LOG2E : -__builtin_huge_valf();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (2 * c >= nt) break;                                     // uniform over the workgroup
        ea_stage_rm<false>(qrm, gq[c], gq[c], nullptr, Ts, tid, c);
        ea_stage_rm<true>(dorm, gdo[c], go[c], dels, Ts, tid, c);
        __syncthreads();
        if (tid < 256) ea_transpose(qt, qrm, c, tid, 0, 4);         // wave-uniform split: four waves per image
        else ea_transpose(dot, dorm, c, tid - 256, 0, 4);
        __syncthreads();
        if (c == 0) OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 2, g < 256);
        if (wave_live) {
          tile(2 * c);
          if (2 * c + 1 < nt) tile(2 * c + 1);
        }
      }
    }
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 3, g < 256);
    __syncthreads();
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 4, g < 256);
    if (wave_live) {
      ea_store_rows(dk, p.scale, keyok, qrm + 32 * wid * EA_HS, p.dk + (int64_t)b * p.k_bs + h * EA_DK, p.k_ts, o0 + 32 * wid, T, lane);
      ea_store_rows(dv, 1.f, keyok, dorm + 32 * wid * EA_HS, p.dv + (int64_t)b * p.v_bs + h * EA_DK, p.v_ts, o0 + 32 * wid, T, lane);
    }
    OTR_STAMP(p.trace, OTR_KID_ENCATTN + orient, g, 5, g < 256);
  }
}

}  // namespace

// shapes this kernel serves (attention.hip asks before it takes its own path)
bool encattn_bwd_takes(int dtype_is_h16, int dk, int Tq, int Tk, int causal, int has_bias, int vec) {
  return dtype_is_h16 && dk == EA_DK && Tq == Tk && Tq >= 1 && Tq <= EA_TMAX && !causal && !has_bias && vec;
}

int32_t encattn_bwd_launch(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, const uint8_t* key_mask,
                           void* dq, void* dk, void* dv, int B, int H, int T, int64_t q_bs, int64_t q_ts, int64_t k_bs, int64_t k_ts, int64_t v_bs,
                           int64_t v_ts, int64_t o_bs, int64_t o_ts, float scale, hipStream_t stream) {
  EaArgs p{};
  p.trace = g_otr_trace;
  p.q = (const uint16_t*)q; p.k = (const uint16_t*)k; p.v = (const uint16_t*)v; p.o = (const uint16_t*)o; p.do_ = (const uint16_t*)do_;
  p.dq = (uint16_t*)dq; p.dk = (uint16_t*)dk; p.dv = (uint16_t*)dv; p.key_mask = key_mask; p.lse = lse;
  p.B = B; p.H = H; p.T = T; p.q_bs = q_bs; p.q_ts = q_ts; p.k_bs = k_bs; p.k_ts = k_ts; p.v_bs = v_bs; p.v_ts = v_ts; p.o_bs = o_bs; p.o_ts = o_ts;
  p.scale = scale;
  if (T <= EA_T) {
    const unsigned grid = 8u * 2u * (unsigned)((H * B + 7) / 8);
    hipLaunchKernelGGL(encattn_bwd_kernel<false>, dim3(grid), dim3(512), 0, stream, p);
  } else {
    const unsigned nob = (unsigned)((T + EA_T - 1) / EA_T);
    const unsigned grid = 8u * 2u * nob * (unsigned)((H * B + 7) / 8);
    hipLaunchKernelGGL(encattn_bwd_kernel<true>, dim3(grid), dim3(512), 0, stream, p);
  }
  return otr_check_launch("encattn_bwd");
}
