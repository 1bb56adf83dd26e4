// Batched edit distance for WER / CER scoring: hypothesis (b, n) of an n-best against reference b, the distance, the substitution /
// deletion / insertion counts of one canonical alignment, and the corpus totals.  Integer only, identical in both builds;
// include/otrans_hip.h states the semantics.
//  * one workgroup per utterance, one wave per pair (the waves of a workgroup take n = wave, wave + waves, ...), so the utterance's
//    totals need no second launch: after a barrier thread 0 adds them with seven 64-bit atomics.
//  * a cell is one 64-bit word, cost << 36 | S << 24 | D << 12 | I (each count <= 2048 < 2^12), so "one substitution more" is one add.
//    Column j of the current row and hypothesis token j live in LDS at [j], touched by lane (j & 63) only: the LDS is per-lane
//    storage, no lane reads what another wrote, and the row loop has no barrier.
//  * a row runs over the columns in chunks of 64.  Lane-local: E[j] = min(diag + c, up + 1), the diagonal winning ties (diag comes from
//    the lane below, for lane 0 from the chunk before).  The left neighbour is a scan: D[i][j] = j + min_{k <= j}(E[k] - k), ties to
//    the largest k, taken as a min-scan of the key ((E[k] - k + 2048) << 12 | 4095 - k) in six shuffle steps, then competing with the
//    carry of the chunks before under the same rule; the cell is E[k]'s plus (j - k) insertions, fetched from lane k by one shuffle.
//  * the reference token of a row is wave-uniform: 64 rows' tokens are loaded at once, one per lane, and broadcast row by row.
#include "common.h"

constexpr int ED_MAX_LEN = 2048;    // widest reference / hypothesis (include/otrans_hip.h)
constexpr int ED_MAX_N = 32;        // most hypotheses per utterance
constexpr int ED_MAX_WAVES = 16;
constexpr int ED_LDS = 65536;       // the largest workgroup allocation that launches without raising the kernel's attribute
constexpr int ED_HDR = 256;         // front of the dynamic block: the pairs' distances [32] and hypothesis 0's counts [3] (no static LDS)
constexpr uint64_t ED_SUB = (1ull << 36) | (1ull << 24), ED_DEL = (1ull << 36) | (1ull << 12), ED_INS = (1ull << 36) | 1ull;
constexpr uint32_t ED_BIAS = 2048;  // E[k] - k >= -k >= -2048

__global__ __launch_bounds__(ED_MAX_WAVES * 64) void edit_distance_kernel(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len,
                                                                          const int64_t* hyp, int64_t hyp_bs, int64_t hyp_ns,
                                                                          const int32_t* hyp_len, int N, int Lr, int Lh, int eos,
                                                                          int lhc, int32_t* dist, int32_t* counts,
                                                                          unsigned long long* totals) {
  extern __shared__ __attribute__((aligned(16))) char ed_smem[];
  int* s_dist = (int*)ed_smem;                                    // [ED_MAX_N]
  int* s_cnt0 = s_dist + ED_MAX_N;                                // [3]
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t* cell = (uint64_t*)(ed_smem + ED_HDR) + (size_t)wave * 2 * lhc;   // [lhc] the row, column j + 1 at [j]
  int64_t* htok = (int64_t*)(cell + lhc);                         // [lhc] hypothesis tokens
  const int R = ref_len[b];
  const bool ref_ok = R >= 0 && R <= Lr;
  const int64_t* rb = ref + (int64_t)b * ref_bs;

  for (int n = wave; n < N; n += nw) {
    const int Hraw = hyp_len[(int64_t)b * N + n];
    int32_t* cn = counts + ((int64_t)b * N + n) * 3;
    if (!ref_ok || Hraw < 0 || Hraw > Lh) {                       // invalid pair: nothing of it is read
      if (lane == 0) {
        dist[(int64_t)b * N + n] = -1;
        cn[0] = cn[1] = cn[2] = -1;
        s_dist[n] = -1;
      }
      continue;
    }
    const int64_t* hb = hyp + (int64_t)b * hyp_bs + (int64_t)n * hyp_ns;
    // tokens and row 0 (j insertions); the hypothesis ends before its first eos.  c0 < Hraw <= Lh <= lhc: every index is inside.
    int H = Hraw;
    for (int c0 = 0; c0 < Hraw; c0 += 64) {
      const int j = c0 + lane;
      const int64_t t = j < Hraw ? hb[j] : 0;
      htok[j] = t;
      cell[j] = (uint64_t)(j + 1) * ED_INS;
      if (eos >= 0) {
        const uint64_t m = __ballot(j < Hraw && t == (int64_t)eos);
        if (m) {
          H = c0 + __ffsll((unsigned long long)m) - 1;
          break;
        }
      }
    }
    const int nch = (H + 63) >> 6;                                // columns past H in the last chunk are computed and never used

    unsigned long long rtok64 = 0;
    for (int i = 1; i <= R; ++i) {
      if (((i - 1) & 63) == 0) rtok64 = (i - 1 + lane < R) ? (unsigned long long)rb[i - 1 + lane] : 0ull;
      const int64_t rt = (int64_t)__shfl(rtok64, (i - 1) & 63);
      uint64_t diag_carry = (uint64_t)(i - 1) * ED_DEL;           // cell (i-1, 0)
      uint32_t key_carry = ((uint32_t)i + ED_BIAS) << 12 | 4095u; // k = 0: E[0] = D[i][0] = i deletions
      uint64_t src_carry = (uint64_t)i * ED_DEL;
      for (int c = 0; c < nch; ++c) {
        const int j = c * 64 + lane + 1;
        const uint64_t up = cell[j - 1];
        unsigned long long dg = __shfl_up((unsigned long long)up, 1);
        if (lane == 0) dg = diag_carry;
        diag_carry = __shfl((unsigned long long)up, 63);
        const uint64_t ed = dg + (htok[j - 1] == rt ? 0ull : ED_SUB), eu = up + ED_DEL;
        const uint64_t e = (ed >> 36) <= (eu >> 36) ? ed : eu;
        uint32_t key = ((uint32_t)(e >> 36) + ED_BIAS - (uint32_t)j) << 12 | (uint32_t)(4095 - j);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = __shfl_up(key, o);
          if (lane >= o) key = min(key, t);
        }
        const bool from_carry = key_carry < key;
        const uint32_t kf = from_carry ? key_carry : key;
        const int k = 4095 - (int)(kf & 4095u);
        unsigned long long src = __shfl((unsigned long long)e, (k - 1) & 63);
        if (from_carry) src = src_carry;
        cell[j - 1] = src + (uint64_t)(j - k) * ED_INS;
        key_carry = __shfl(kf, 63);
        src_carry = __shfl(src, 63);
      }
    }
    if (lane == (H > 0 ? (H - 1) & 63 : 0)) {                     // the lane that owns column H writes the pair's result
      const uint64_t fin = H > 0 ? cell[H - 1] : (uint64_t)R * ED_DEL;
      const int d = (int)(fin >> 36), cs = (int)(fin >> 24) & 4095, cd = (int)(fin >> 12) & 4095, ci = (int)fin & 4095;
      dist[(int64_t)b * N + n] = d;
      cn[0] = cs; cn[1] = cd; cn[2] = ci;
      s_dist[n] = d;
      if (n == 0) { s_cnt0[0] = cs; s_cnt0[1] = cd; s_cnt0[2] = ci; }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_dist[0] < 0) {                                          // covers a bad reference: every pair of it is -1
      atomicAdd(totals + 7, 1ull);
    } else {
      int best = s_dist[0];
      for (int n = 1; n < N; ++n)
        if (s_dist[n] >= 0) best = min(best, s_dist[n]);
      atomicAdd(totals + 0, 1ull);
      atomicAdd(totals + 1, (unsigned long long)R);
      atomicAdd(totals + 2, (unsigned long long)s_dist[0]);
      atomicAdd(totals + 3, (unsigned long long)s_cnt0[0]);
      atomicAdd(totals + 4, (unsigned long long)s_cnt0[1]);
      atomicAdd(totals + 5, (unsigned long long)s_cnt0[2]);
      atomicAdd(totals + 6, (unsigned long long)best);
    }
  }
}

extern "C" int32_t otr_edit_distance(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len, const int64_t* hyp, int64_t hyp_bs,
                                     int64_t hyp_ns, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Lr, int32_t Lh,
                                     int32_t eos, int32_t* dist, int32_t* counts, int64_t* totals, void* stream) {
  OTR_REQUIRE(B >= 0, "edit_distance: B=%d must be >= 0", B);
  OTR_REQUIRE(N >= 1 && N <= ED_MAX_N, "edit_distance: N=%d hypotheses per utterance, 1 .. %d supported", N, ED_MAX_N);
  OTR_REQUIRE(Lr >= 0 && Lr <= ED_MAX_LEN && Lh >= 0 && Lh <= ED_MAX_LEN, "edit_distance: widths Lr=%d Lh=%d, 0 .. %d supported", Lr,
              Lh, ED_MAX_LEN);
  OTR_REQUIRE(eos >= -1, "edit_distance: eos=%d must be a token id or -1", eos);
  OTR_REQUIRE(ref_bs >= 0 && hyp_bs >= 0 && hyp_ns >= 0, "edit_distance: negative stride");
  if (B == 0) return 0;
  OTR_REQUIRE(ref_len && hyp_len && dist && counts && totals && (ref || Lr == 0) && (hyp || Lh == 0), "edit_distance: null pointer");
  OTR_REQUIRE(((uintptr_t)totals & 7) == 0, "edit_distance: totals must be 8-byte aligned");
  const int lhc = Lh == 0 ? 64 : ((Lh + 63) / 64) * 64;           // 16 bytes of LDS per column and wave
  int nw = (ED_LDS - ED_HDR) / (16 * lhc);                        // 1 at 2048 columns, 15 up to 256
  nw = nw < N ? nw : N;
  nw = nw < ED_MAX_WAVES ? nw : ED_MAX_WAVES;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(B), dim3(nw * 64), ED_HDR + (size_t)nw * 16 * lhc, (hipStream_t)stream, ref, ref_bs, ref_len,
                     hyp, hyp_bs, hyp_ns, hyp_len, N, Lr, Lh, eos, lhc, dist, counts, (unsigned long long*)totals);
  return otr_check_launch("edit_distance");
}
