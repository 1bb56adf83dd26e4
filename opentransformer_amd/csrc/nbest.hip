// Per-token edit alignment and the consensus of an n-best: which hypothesis token is a match, a substitution or an insertion (and
// against which reference token), the expected edit distance of every hypothesis under the n-best's posterior (its risk, for minimum
// Bayes risk decoding) and the posterior mass that agrees with each of its tokens (its confidence).  Integer alignment, f32 sums in a
// fixed order; no 16-bit operand, identical in both builds; include/otrans_hip.h states the semantics.
//  * one wave per pair.  The row sweep is editdist.hip's: 64-column chunks, E[j] = min(diag + c, up + 1) with the diagonal winning
//    ties (diag from the lane below, for lane 0 from the chunk before), the left neighbour as a min-scan of the key
//    ((E[k] - k + 2048) << 12 | 4095 - k), ties to the largest k.  A cell here is the cost alone (the counts come from the walk), so
//    D[i][j] is read off the winning key and no second shuffle fetches lane k's cell.
//  * back-pointers: per row and chunk two 64-bit ballots, `up` (the cell came from above) and `left` (k != j: from the left); neither
//    bit: the diagonal.  16 bytes per row and chunk, 16 KB for a 256 x 256 pair: they stay in LDS, which is what bounds the widths.
//  * the walk back from (R, H) is serial and short (at most R + H steps): lane 0 reads the ballot words of its cell and writes the
//    reference index of each hypothesis token over the cost row, -1 for an insertion; match or substitution is then one parallel
//    compare.
//  * consensus: one workgroup per (utterance, hypothesis i), its waves take the references j = wave, wave + waves, ...; a pair leaves
//    its distance and the ballots of its matching tokens in LDS, and after a barrier thread k sums post[j] over j ascending for token
//    k and thread 0 the risk: the order is fixed, nothing is added atomically.  A second, tiny launch picks the least risk.
#include "common.h"

constexpr int NB_MAX_LEN = 256;     // widest hypothesis / reference (include/otrans_hip.h OTR_NBEST_MAX_LEN)
constexpr int NB_MAX_N = 32;        // most hypotheses per utterance
constexpr int NB_MAX_WAVES = 16;
constexpr int NB_LDS = 65536;       // the largest workgroup allocation that launches without raising the kernel's attribute
constexpr int NB_CH = NB_MAX_LEN / 64;
constexpr uint32_t NB_BIAS = 2048;  // E[k] - k >= -k >= -256
static_assert(OTR_NBEST_MAX_LEN == NB_MAX_LEN, "the header's limit is this file's");

__device__ __forceinline__ void nb_wave_sync() {   // LDS written by one lane of the wave, read by another
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// where the sequence ends: before the first eos among its first n tokens (eos >= 0), else n.  Wave-uniform.
__device__ int nb_cut(const int64_t* t, int n, int eos, int lane) {
  if (eos < 0) return n;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int j = c0 + lane;
    const uint64_t m = __ballot(j < n && t[j] == (int64_t)eos);
    if (m) return c0 + __ffsll((unsigned long long)m) - 1;
  }
  return n;
}

// One pair: hypothesis htok[0, H) (LDS, readable up to the next multiple of 64) against reference rb[0, R) (global).  row: [>= 64 *
// chunks of H] ints of LDS, bp: [R * chunks * 2] 64-bit words of LDS, both this wave's own.  Returns D[R][H] and leaves in row[j] the
// reference index hypothesis token j is aligned to (match or substitution), -1 for an insertion, j < H.
__device__ int nb_align_pair(const int64_t* rb, int R, const int64_t* htok, int H, int* row, uint64_t* bp, int lane) {
  const int nch = (H + 63) >> 6;
  for (int c = 0; c < nch; ++c) row[c * 64 + lane] = c * 64 + lane + 1;       // row 0: j insertions
  unsigned long long rtok64 = 0;
  for (int i = 1; i <= R; ++i) {
    if (((i - 1) & 63) == 0) rtok64 = (i - 1 + lane < R) ? (unsigned long long)rb[i - 1 + lane] : 0ull;
    const int64_t rt = (int64_t)__shfl(rtok64, (i - 1) & 63);
    int diag_carry = i - 1;                                                   // cell (i-1, 0)
    uint32_t key_carry = ((uint32_t)i + NB_BIAS) << 12 | 4095u;               // k = 0: E[0] = D[i][0] = i deletions
    for (int c = 0; c < nch; ++c) {
      const int j = c * 64 + lane + 1;
      const int up = row[j - 1];
      int dg = __shfl_up(up, 1);
      if (lane == 0) dg = diag_carry;
      diag_carry = __shfl(up, 63);
      const int ed = dg + (htok[j - 1] == rt ? 0 : 1), eu = up + 1;
      const int e = ed <= eu ? ed : eu;
      const uint32_t own = ((uint32_t)e + NB_BIAS - (uint32_t)j) << 12 | (uint32_t)(4095 - j);
      uint32_t key = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(key, o);
        if (lane >= o) key = min(key, t);
      }
      const uint32_t kf = min(key, key_carry);
      const bool left = kf != own;                                            // the keys of different k differ: k < j
      row[j - 1] = (int)(kf >> 12) - (int)NB_BIAS + j;
      const uint64_t m_up = __ballot(!left && ed > eu), m_left = __ballot(left);
      if (lane == 0) {
        bp[((i - 1) * nch + c) * 2] = m_up;
        bp[((i - 1) * nch + c) * 2 + 1] = m_left;
      }
      key_carry = __shfl(kf, 63);
    }
  }
  nb_wave_sync();
  const int dist = H > 0 ? row[H - 1] : R;
  nb_wave_sync();                                                             // every lane has read the corner before the walk overwrites it
  if (lane == 0) {
    int i = R, j = H;
    while (j > 0) {                                                           // from (i, 0) on only deletions are left: no token
      if (i == 0) {
        row[--j] = -1;
        continue;
      }
      const int c = (j - 1) >> 6, bit = (j - 1) & 63;
      if ((bp[((i - 1) * nch + c) * 2 + 1] >> bit) & 1) row[--j] = -1;
      else if ((bp[((i - 1) * nch + c) * 2] >> bit) & 1) --i;
      else row[--j] = --i;
    }
  }
  nb_wave_sync();
  return dist;
}

// the LDS of one wave of a pair kernel: the row, then the back-pointers
__host__ __device__ constexpr size_t nb_wave_bytes(int rows, int lhc) { return (size_t)lhc * 4 + (size_t)(rows > 0 ? rows : 1) * (lhc / 64) * 16; }

__global__ __launch_bounds__(64) void edit_align_kernel(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len, const int64_t* hyp,
                                                        int64_t hyp_bs, int64_t hyp_ns, const int32_t* hyp_len, int N, int Lr, int Lh,
                                                        int eos, int lhc, int32_t* dist, int8_t* code, int32_t* ref_pos) {
  extern __shared__ __attribute__((aligned(16))) char nb_smem[];
  int64_t* htok = (int64_t*)nb_smem;                              // [lhc]
  uint64_t* bp = (uint64_t*)(htok + lhc);                         // [Lr * lhc / 64 * 2]
  int* row = (int*)(bp + (size_t)(Lr > 0 ? Lr : 1) * (lhc / 64) * 2);   // [lhc]
  const int b = blockIdx.x / N, n = blockIdx.x % N, lane = threadIdx.x;
  const int64_t pair = (int64_t)b * N + n;
  const int R = ref_len[b], Hraw = hyp_len[pair];
  int8_t* cd = code + pair * Lh;
  int32_t* rp = ref_pos + pair * Lh;
  if (R < 0 || R > Lr || Hraw < 0 || Hraw > Lh) {                 // invalid pair: nothing of it is read
    if (lane == 0) dist[pair] = -1;
    for (int j = lane; j < Lh; j += 64) { cd[j] = -1; rp[j] = -1; }
    return;
  }
  const int64_t* rb = ref + (int64_t)b * ref_bs;
  const int64_t* hb = hyp + (int64_t)b * hyp_bs + (int64_t)n * hyp_ns;
  const int H = nb_cut(hb, Hraw, eos, lane);
  for (int j = lane; j < lhc; j += 64) htok[j] = j < H ? hb[j] : 0;   // lane-private: lane (j & 63) alone reads htok[j] in the sweep
  const int d = nb_align_pair(rb, R, htok, H, row, bp, lane);
  if (lane == 0) dist[pair] = d;
  for (int j = lane; j < Lh; j += 64) {
    const int r = j < H ? row[j] : -1;
    cd[j] = j >= H ? -1 : r < 0 ? 2 : htok[j] == rb[r] ? 0 : 1;
    rp[j] = r;
  }
}

// a slot takes part if its score is finite and its length fits the width
__device__ __forceinline__ bool nb_live(float score, int len, int L) { return isfinite(score) && len >= 0 && len <= L; }

__global__ __launch_bounds__(NB_MAX_WAVES * 64) void nbest_consensus_kernel(const int64_t* tokens, int64_t tok_bs, int64_t tok_ns,
                                                                            const int32_t* lengths, const float* scores, float scale,
                                                                            int N, int L, int eos, int lhc, float* post, float* risk,
                                                                            float* conf) {
  extern __shared__ __attribute__((aligned(16))) char nb_smem[];
  __shared__ uint64_t s_match[NB_MAX_N][NB_CH];                   // the matching tokens of hypothesis i against reference j
  __shared__ float s_post[NB_MAX_N];
  __shared__ int s_dist[NB_MAX_N];
  __shared__ int s_H;
  int64_t* htok = (int64_t*)nb_smem;                              // [lhc] hypothesis i, shared by the waves (read only after the barrier)
  const int b = blockIdx.x / N, i = blockIdx.x % N, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int nchl = lhc / 64;
  char* mine = nb_smem + (size_t)lhc * 8 + (size_t)wave * nb_wave_bytes(L, lhc);
  uint64_t* bp = (uint64_t*)mine;                                 // [L * nchl * 2]
  int* row = (int*)(mine + (size_t)(L > 0 ? L : 1) * nchl * 16);  // [lhc]
  const int64_t* tb = tokens + (int64_t)b * tok_bs;
  const int32_t* lb = lengths + (int64_t)b * N;
  const float* sb = scores + (int64_t)b * N;
  float* cf = conf + ((int64_t)b * N + i) * L;

  if (wave == 0) {
    // post = softmax over the live slots of scale * score, as exp(scale * (score - pivot)) with the pivot the slot of the largest
    // scale * score: the difference of two nearby scores is exact, so the rounding of a large |score| never reaches the exponent
    const bool live = lane < N && nb_live(sb[lane < N ? lane : 0], lb[lane < N ? lane : 0], L);
    const float s = live ? sb[lane] : 0.f;
    const float pivot = scale >= 0.f ? wave_max(live ? s : -INFINITY) : -wave_max(live ? -s : -INFINITY);
    const float e = live ? expf(scale * (s - pivot)) : 0.f;
    if (lane < N) s_post[lane] = e;
    nb_wave_sync();
    float sum = 0.f;
    for (int j = 0; j < N; ++j) sum += s_post[j];                 // every lane the same sum, j ascending
    nb_wave_sync();
    if (lane < N) s_post[lane] = live ? e / sum : 0.f;
    const int Hi = lb[i];
    const int H = (Hi >= 0 && Hi <= L) ? nb_cut(tb + (int64_t)i * tok_ns, Hi, eos, lane) : 0;
    if (lane == 0) s_H = H;
  }
  __syncthreads();
  const int H = s_H;
  const bool live_i = nb_live(sb[i], lb[i], L);                   // uniform over the workgroup
  if (threadIdx.x == 0) post[(int64_t)b * N + i] = s_post[i];
  if (!live_i) {
    if (threadIdx.x == 0) risk[(int64_t)b * N + i] = INFINITY;
    for (int k = threadIdx.x; k < L; k += blockDim.x) cf[k] = 0.f;
    return;
  }
  {
    const int64_t* hb = tb + (int64_t)i * tok_ns;
    for (int j = threadIdx.x; j < lhc; j += blockDim.x) htok[j] = j < H ? hb[j] : 0;
  }
  __syncthreads();

  for (int j = wave; j < N; j += nw) {
    if (!nb_live(sb[j], lb[j], L)) continue;                      // wave-uniform
    if (j == i) {                                                 // against itself: every token matches
      if (lane < nchl) s_match[j][lane] = H >= (lane + 1) * 64 ? ~0ull : H > lane * 64 ? (1ull << (H - lane * 64)) - 1 : 0ull;
      if (lane == 0) s_dist[j] = 0;
      continue;
    }
    const int64_t* rb = tb + (int64_t)j * tok_ns;
    const int R = nb_cut(rb, lb[j], eos, lane);
    const int d = nb_align_pair(rb, R, htok, H, row, bp, lane);
    for (int c = 0; c < nchl; ++c) {
      const int k = c * 64 + lane;
      const int r = k < H ? row[k] : -1;
      const uint64_t m = __ballot(r >= 0 && htok[k] == rb[r]);
      if (lane == 0) s_match[j][c] = m;
    }
    if (lane == 0) s_dist[j] = d;
    nb_wave_sync();                                               // the row is read before the next pair's sweep writes it
  }
  __syncthreads();

  for (int k = threadIdx.x; k < L; k += blockDim.x) {
    float acc = 0.f;
    if (k < H)
      for (int j = 0; j < N; ++j)                                 // a dead slot left no masks
        if (nb_live(sb[j], lb[j], L) && ((s_match[j][k >> 6] >> (k & 63)) & 1)) acc += s_post[j];
    cf[k] = acc;
  }
  if (threadIdx.x == 0) {
    double acc = 0.0;                                             // 32 products of a distance up to 256: exact until the one rounding
    for (int j = 0; j < N; ++j)
      if (nb_live(sb[j], lb[j], L)) acc += (double)s_post[j] * (double)s_dist[j];
    risk[(int64_t)b * N + i] = (float)acc;
  }
}

// best[b]: the live slot of least risk, ties to the higher score, then the lower index; -1 without a live slot
__global__ void nbest_best_kernel(const int32_t* lengths, const float* scores, const float* risk, int B, int N, int L, int32_t* best) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int arg = -1;
  float r0 = 0.f, s0 = 0.f;
  for (int j = 0; j < N; ++j) {
    const float s = scores[(int64_t)b * N + j], r = risk[(int64_t)b * N + j];
    if (!nb_live(s, lengths[(int64_t)b * N + j], L)) continue;
    if (arg < 0 || r < r0 || (r == r0 && s > s0)) { arg = j; r0 = r; s0 = s; }
  }
  best[b] = arg;
}

extern "C" int32_t otr_edit_align(const int64_t* ref, int64_t ref_bs, const int32_t* ref_len, const int64_t* hyp, int64_t hyp_bs,
                                  int64_t hyp_ns, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Lr, int32_t Lh, int32_t eos,
                                  int32_t* dist, int8_t* code, int32_t* ref_pos, void* stream) {
  OTR_REQUIRE(B >= 0 && B <= (1 << 20), "edit_align: B=%d must be in [0, 2^20]", B);
  OTR_REQUIRE(N >= 1 && N <= NB_MAX_N, "edit_align: N=%d hypotheses per utterance, 1 .. %d supported", N, NB_MAX_N);
  OTR_REQUIRE(Lr >= 0 && Lr <= NB_MAX_LEN && Lh >= 0 && Lh <= NB_MAX_LEN, "edit_align: widths Lr=%d Lh=%d, 0 .. %d supported", Lr, Lh,
              NB_MAX_LEN);
  OTR_REQUIRE(eos >= -1, "edit_align: eos=%d must be a token id or -1", eos);
  OTR_REQUIRE(ref_bs >= 0 && hyp_bs >= 0 && hyp_ns >= 0, "edit_align: negative stride");
  if (B == 0) return 0;
  OTR_REQUIRE(ref_len && hyp_len && dist && (code || Lh == 0) && (ref_pos || Lh == 0) && (ref || Lr == 0) && (hyp || Lh == 0),
              "edit_align: null pointer");
  const int lhc = Lh == 0 ? 64 : ((Lh + 63) / 64) * 64;
  hipLaunchKernelGGL(edit_align_kernel, dim3(B * N), dim3(64), (size_t)lhc * 8 + nb_wave_bytes(Lr, lhc), (hipStream_t)stream, ref, ref_bs,
                     ref_len, hyp, hyp_bs, hyp_ns, hyp_len, N, Lr, Lh, eos, lhc, dist, code, ref_pos);
  return otr_check_launch("edit_align");
}

extern "C" int32_t otr_nbest_consensus(const int64_t* tokens, int64_t tok_bs, int64_t tok_ns, const int32_t* lengths, const float* scores,
                                       float scale, int32_t B, int32_t N, int32_t L, int32_t eos, float* post, float* risk,
                                       int32_t* best, float* conf, void* stream) {
  OTR_REQUIRE(B >= 0 && B <= (1 << 20), "nbest_consensus: B=%d must be in [0, 2^20]", B);
  OTR_REQUIRE(N >= 1 && N <= NB_MAX_N, "nbest_consensus: N=%d hypotheses per utterance, 1 .. %d supported", N, NB_MAX_N);
  OTR_REQUIRE(L >= 0 && L <= NB_MAX_LEN, "nbest_consensus: width L=%d, 0 .. %d supported", L, NB_MAX_LEN);
  OTR_REQUIRE(eos >= -1, "nbest_consensus: eos=%d must be a token id or -1", eos);
  OTR_REQUIRE(tok_bs >= 0 && tok_ns >= 0, "nbest_consensus: negative stride");
  OTR_REQUIRE(scale == scale && scale - scale == 0.f, "nbest_consensus: scale must be finite");
  if (B == 0) return 0;
  OTR_REQUIRE(lengths && scores && post && risk && best && (conf || L == 0) && (tokens || L == 0), "nbest_consensus: null pointer");
  const int lhc = L == 0 ? 64 : ((L + 63) / 64) * 64;
  int nw = (int)((NB_LDS - 2048 - (size_t)lhc * 8) / nb_wave_bytes(L, lhc));   // 2048: the static arrays; 3 waves at 256 columns
  nw = nw < N ? nw : N;
  nw = nw < NB_MAX_WAVES ? nw : NB_MAX_WAVES;
  hipLaunchKernelGGL(nbest_consensus_kernel, dim3(B * N), dim3(nw * 64), (size_t)lhc * 8 + (size_t)nw * nb_wave_bytes(L, lhc),
                     (hipStream_t)stream, tokens, tok_bs, tok_ns, lengths, scores, scale, N, L, eos, lhc, post, risk, conf);
  int32_t rc = otr_check_launch("nbest_consensus");
  if (rc) return rc;
  hipLaunchKernelGGL(nbest_best_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, lengths, scores, risk, B, N, L, best);
  return otr_check_launch("nbest_best");
}
