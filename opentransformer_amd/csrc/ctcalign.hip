// CTC forced alignment: the most probable CTC path of a known label sequence (Viterbi over the extended states of the loss, the
// max-plus twin of the alpha recursion in ctc.hip), its per-frame tokens, per-label frame spans, per-label log-probs and score.
// One launch per batch, f32 in both builds; include/otrans_hip.h states the semantics.
//  * one workgroup per utterance, one thread per extended state s (S = 2L+1 <= 255).  The workgroup has as many waves as the widest
//    utterance the caller allows (2 max_tgt + 1 states rounded up to 64), not always four: at ~20 labels one wave runs the frame loop
//    and the per-frame barrier costs nothing.
//  * the previous frame lives in a double-buffered LDS row (one barrier per frame).  The gather x_t(ext(s)) does not depend on the
//    recurrence: it is issued CA_PF frames ahead into registers, so the per-frame chain is LDS exchange + max + add.
//  * back-pointers (step 0 / 1 / 2, two bits per (t, s)) are packed by two wave ballots per wave and frame into 64 B per frame:
//    word (t*4 + wave)*2 + bit.  They stay in LDS while T <= CA_LDS_T (header + T * 64 B <= 64 KiB: the largest workgroup allocation
//    that launches without raising the kernel's dynamic-LDS attribute, and one that leaves two workgroups per CU resident); above
//    that they go to the caller's workspace.
//  * lane 0 walks the back-pointers once (T dependent reads) and leaves the frame -> state map in frame_token; three parallel passes
//    turn it into spans (first / one-past-last frame of each label state), tokens, and the per-label sums (ascending t).
#include "common.h"

#define NEG_INF (-__builtin_huge_valf())

constexpr int CA_NT = 256;          // most threads of a workgroup: 255 states
constexpr int CA_PF = 16;           // frames of gathered log-probs in flight
constexpr int CA_LDS_T = 960;       // back-pointers in LDS up to this T (include/otrans_hip.h states it)
constexpr int CA_HDR = 2 * CA_NT * 4 + 2 * 128 * 4 + 64;   // LDS in front of the back-pointers: two state rows, span ends, end state

template <bool BP_LDS>
__global__ __launch_bounds__(CA_NT) void ctc_align_kernel(const float* lp, int64_t ld, const int64_t* targets, int64_t ldt,
                                                          const int32_t* in_len, const int32_t* tgt_len, int T, int V,
                                                          int max_tgt, int blank, uint64_t* ws, int32_t* frame_token, int32_t* spans,
                                                          float* label_logp, float* score) {
  extern __shared__ __attribute__((aligned(16))) char ca_smem[];
  float* sh = (float*)ca_smem;                                    // [2][CA_NT]
  int* s_first = (int*)(ca_smem + 2 * CA_NT * 4);                 // [128]
  int* s_last = s_first + 128;                                    // [128]
  int* s_end = s_last + 128;                                      // the path's last state, -1: infeasible
  uint64_t* bp = BP_LDS ? (uint64_t*)(ca_smem + CA_HDR) : ws + (int64_t)blockIdx.x * T * 8;
  const int b = blockIdx.x, s = threadIdx.x, nt = blockDim.x;
  const int Lraw = tgt_len[b];
  const bool bad_len = Lraw < 0 || Lraw > max_tgt;               // never computed: `targets` holds max_tgt labels per row
  const int Tb = max(min(in_len[b], T), 0), L = bad_len ? 0 : Lraw, S = 2 * L + 1;
  const float* lpb = lp + (int64_t)b * T * ld;
  const int64_t* tg = targets + (int64_t)b * ldt;
  int32_t* ft = frame_token + (int64_t)b * T;
  int32_t* sp = spans + (int64_t)b * max_tgt * 2;
  float* ll = label_logp + (int64_t)b * max_tgt;
  const bool live = s < S;
  const int ext = (live && (s & 1)) ? (int)tg[s >> 1] : blank;
  const int ext_m2 = (live && s >= 2 && (s & 1)) ? (int)tg[(s - 2) >> 1] : blank;
  const bool skip = live && s >= 2 && ext != blank && ext != ext_m2;          // s-2 -> s allowed, as in the loss
  const int wave = s >> 6, lane = s & 63;
  const bool wave_live = wave * 64 < S;

  for (int e = s; e < max_tgt; e += nt) { sp[2 * e] = -1; sp[2 * e + 1] = -1; ll[e] = 0.f; }
  // a bad length or a label outside [0, V) (its gather would leave the row): infeasible, nothing of it is computed
  if (__syncthreads_or(bad_len || ext < 0 || ext >= V)) {
    for (int t = s; t < T; t += nt) ft[t] = -1;
    if (s == 0) score[b] = NEG_INF;
    return;
  }
  for (int t = Tb + s; t < T; t += nt) ft[t] = -1;

  // ---------------- best-path scores, frame by frame
  float v = NEG_INF;
  if (Tb > 0) {
    if (s == 0) v = lpb[blank];
    else if (s == 1 && S > 1) v = lpb[ext];
  }
  sh[s] = v;
  float xa[CA_PF], xb[CA_PF];
  auto gather = [&](float (&x)[CA_PF], int t0) {
#pragma unroll
    for (int i = 0; i < CA_PF; ++i) x[i] = (live && t0 + i < Tb) ? lpb[(int64_t)(t0 + i) * ld + ext] : 0.f;
  };
  auto frames = [&](const float (&x)[CA_PF], int t0) {
#pragma unroll
    for (int i = 0; i < CA_PF; ++i) {
      const int t = t0 + i;
      if (t >= Tb) break;                                         // Tb is uniform over the workgroup
      __syncthreads();
      const float* prev = sh + ((t - 1) & 1) * CA_NT;
      const float a1 = s >= 1 ? prev[s - 1] : NEG_INF;
      const float a2 = skip ? prev[s - 2] : NEG_INF;
      float m = prev[s];
      int k = 0;                                                  // equal predecessors: the smallest step wins
      if (a1 > m) { m = a1; k = 1; }
      if (a2 > m) { m = a2; k = 2; }
      sh[(t & 1) * CA_NT + s] = live ? m + x[i] : NEG_INF;
      const uint64_t b0 = __ballot(k & 1), b1 = __ballot(k >> 1);
      if (lane == 0 && wave_live) {
        bp[((int64_t)t * 4 + wave) * 2] = b0;
        bp[((int64_t)t * 4 + wave) * 2 + 1] = b1;
      }
    }
  };
  gather(xa, 1);
  for (int t0 = 1; t0 < Tb; t0 += 2 * CA_PF) {
    gather(xb, t0 + CA_PF);
    frames(xa, t0);
    gather(xa, t0 + 2 * CA_PF);
    frames(xb, t0 + CA_PF);
  }
  __syncthreads();

  // ---------------- the end state, then the back-trace by one lane
  if (s == 0) {
    int end = -1;
    float best = NEG_INF;
    if (Tb == 0) {
      if (L == 0) { best = 0.f; }                                 // no frames, no labels: the empty path
    } else {
      const float* fin = sh + ((Tb - 1) & 1) * CA_NT;
      const float v2 = fin[S - 1], v1 = S > 1 ? fin[S - 2] : NEG_INF;
      best = v2; end = S - 1;                                     // the final blank wins a tie
      if (v1 > v2) { best = v1; end = S - 2; }
      if (best == NEG_INF) end = -1;
    }
    score[b] = best;
    *s_end = end;
    if (end >= 0) {
      int st = end;
      for (int t = Tb - 1; t >= 1; --t) {
        ft[t] = st;
        const uint64_t* w = bp + ((int64_t)t * 4 + (st >> 6)) * 2;
        const uint64_t w0 = w[0], w1 = w[1];
        st -= (int)((w0 >> (st & 63)) & 1) + 2 * (int)((w1 >> (st & 63)) & 1);
      }
      ft[0] = st;
    }
  }
  for (int e = s; e < 256; e += nt) s_first[e] = -1;              // s_first and s_last, adjacent
  __syncthreads();
  if (*s_end < 0) {                                               // infeasible (or no frames): no path
    for (int t = s; t < Tb; t += nt) ft[t] = -1;
    return;
  }
  // ---------------- frame -> state map (in frame_token) -> spans, tokens, per-label sums
  for (int t = s; t < Tb; t += nt) {
    const int st = ft[t];
    if (st & 1) {
      if (t == 0 || ft[t - 1] != st) s_first[st >> 1] = t;
      if (t + 1 == Tb || ft[t + 1] != st) s_last[st >> 1] = t + 1;
    }
  }
  __syncthreads();
  for (int t = s; t < Tb; t += nt) {
    const int st = ft[t];
    ft[t] = (st & 1) ? (int)tg[st >> 1] : blank;
  }
  for (int j = s; j < L; j += nt) {
    const int t0 = s_first[j], t1 = s_last[j];
    const int c = (int)tg[j];
    float acc = 0.f;
    for (int t = t0; t < t1; ++t) acc += lpb[(int64_t)t * ld + c];
    sp[2 * j] = t0;
    sp[2 * j + 1] = t1;
    ll[j] = acc;
  }
}

extern "C" int64_t otr_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t max_tgt) {
  if (B < 1 || T < 1 || max_tgt < 0 || max_tgt > 127) return -1;
  return T <= CA_LDS_T ? 8 : (int64_t)B * T * 64;                 // up to CA_LDS_T frames the back-pointers stay in LDS
}

extern "C" int32_t otr_ctc_align(const float* log_probs, int64_t ld, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                                 const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank,
                                 void* workspace, int64_t ws_bytes, int32_t* frame_token, int32_t* spans, float* label_logp,
                                 float* score, void* stream) {
  OTR_REQUIRE(log_probs && targets && in_len && tgt_len && workspace && frame_token && spans && label_logp && score,
              "ctc_align: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1 && V > 1, "ctc_align: bad shape B=%d T=%d V=%d", B, T, V);
  OTR_REQUIRE(max_tgt >= 0 && max_tgt <= 127, "ctc_align: target length %d > 127 not supported", max_tgt);
  OTR_REQUIRE(ld >= V && ldt >= max_tgt, "ctc_align: ld=%lld must be >= V=%d and ldt=%lld >= max_tgt=%d", (long long)ld, V,
              (long long)ldt, max_tgt);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_align: blank=%d must be in [0, V=%d)", blank, V);
  OTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "ctc_align: workspace must be 8-byte aligned");
  const int64_t need = otr_ctc_align_workspace_bytes(B, T, max_tgt);
  OTR_REQUIRE(ws_bytes >= need, "ctc_align: workspace of %lld bytes, %lld needed (otr_ctc_align_workspace_bytes)", (long long)ws_bytes,
              (long long)need);
  const int nt = ((2 * max_tgt + 1 + 63) / 64) * 64;
  hipStream_t s = (hipStream_t)stream;
  if (T <= CA_LDS_T)
    hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(B), dim3(nt), CA_HDR + (size_t)T * 64, s, log_probs, ld, targets, ldt, in_len,
                       tgt_len, T, V, max_tgt, blank, (uint64_t*)workspace, frame_token, spans, label_logp, score);
  else
    hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(B), dim3(nt), CA_HDR, s, log_probs, ld, targets, ldt, in_len, tgt_len, T,
                       V, max_tgt, blank, (uint64_t*)workspace, frame_token, spans, label_logp, score);
  return otr_check_launch("ctc_align");
}
