// CTC segmentation of long recordings: the most probable CTC path of a known label sequence of up to 4095 labels that may start and
// end anywhere in the recording (Kuerzinger et al. 2020), with a charge of skip_logp for every frame it leaves out.  The max-plus
// recursion of ctcalign.hip over up to 8191 extended states, plus a virtual start at states 0 / 1 and an end candidate at every frame.
// One launch per batch, f32 in both builds; include/otrans_hip.h states the semantics.
//  * one workgroup per recording (the frame loop is a serial chain; workgroups never wait for each other).  Each thread holds a strip
//    of R consecutive states in registers, R = 4 up to 2047 labels and 8 above, so the workgroup has ceil(S / R) threads rounded up to
//    a wave: one wave up to 127 labels, 16 waves at either variant's limit.  R is even, so a strip starts at a blank state: the only
//    value that crosses to the right neighbour is the strip's last one (v(s-1) of its blank, v(s-2) of its first label), through a
//    double-buffered LDS row with one barrier per frame.
//  * the gathers x_t(ext(s)) do not depend on the recurrence: R/2 label columns and the one blank column all strips share are issued
//    PF frames ahead into registers (two sets, refilled alternately).  PF is 16 while the workgroup has at most 256 threads (up to 511
//    labels), 6 (R = 4) and 3 (R = 8) at up to 1024 threads, where __launch_bounds__ leaves 128 registers: 121 / 103 / 114 VGPRs, no
//    scratch.
//  * back-pointers are 2 bits per (t, s) -- step 0 / 1 / 2, 3 = the path starts here -- one byte (R = 4) or half-word (R = 8) per thread
//    and frame: state s sits at bits 2 (s & 15) of 32-bit word s >> 4 of the frame's row in the caller's workspace.
//  * the end candidate of frame t needs v_t(2L-1) and v_t(2L); 2L may open a strip, so its owner judges frame t-1 in iteration t, when
//    the neighbour's value has crossed anyway.
//  * back-trace in blocks of 64 frames: a state falls by at most 2 per frame, so the 64 rows of a block matter only in the 9 words
//    around the current state.  64 threads fetch them at once (one global round trip per block) into LDS, thread 0 walks the block
//    there and leaves the states in LDS, 64 threads store them to frame_token.  Three parallel passes turn the frame -> state map
//    into spans, tokens and the per-label sums (ascending t), as in ctcalign.hip.
#include "common.h"

// the header states a multiply and an add of one rounding each (v + float(n) * skip_logp), never one fused multiply-add.  Plain * and +
// below: the __fmul_rn / __fadd_rn of the HIP headers are inline functions compiled under the default contraction and fuse all the same
#pragma clang fp contract(off)

#define NEG_INF (-__builtin_huge_valf())

constexpr int CS_MAX_TGT = 4095;
constexpr int CS_MAX_T = 1 << 20;   // float(t) is exact
constexpr int CS_NT = 1024;         // most threads of a workgroup
constexpr int CS_TB = 64;           // frames of a back-trace block
constexpr int CS_TW = 9;            // 32-bit words of a frame's row a block can touch: 128 states below the current one, 16 per word

static int cs_strip(int max_tgt) { return max_tgt <= 2047 ? 4 : 8; }
static int cs_threads(int max_tgt) {
  const int R = cs_strip(max_tgt), S = 2 * max_tgt + 1;
  return ((S + R - 1) / R + 63) / 64 * 64;
}
static int64_t cs_row_bytes(int max_tgt) { return (int64_t)cs_threads(max_tgt) * cs_strip(max_tgt) / 4; }

template <int R, int PF>
struct CsGather {
  float l[PF][R / 2];   // x_t(label) of the strip's label states
  float b[PF];          // x_t(blank)
};

template <int R, int PF, int NT>
__global__ __launch_bounds__(NT) void ctc_segment_kernel(const float* lp, int64_t ld, const int64_t* targets, int64_t ldt,
                                                         const int32_t* in_len, const int32_t* tgt_len, int T, int V, int max_tgt,
                                                         int blank, int free_start, int free_end, float skip_logp, uint8_t* ws,
                                                         int64_t row_bytes, int32_t* frame_token, int32_t* spans, float* label_logp,
                                                         float* score, int32_t* bounds) {
  constexpr int H = R / 2;
  __shared__ float edge[2][CS_NT + 1];            // [frame parity][1 + thread]: the strip's last value; entry 0 stays -inf
  __shared__ uint32_t tr[CS_TB][CS_TW];           // the back-pointer words of a back-trace block
  __shared__ int path[CS_TB];                     // its states
  __shared__ int s_cur[5];                        // frame, state, done, first frame, steps
  __shared__ float s_best;
  const int b = blockIdx.x, i = threadIdx.x, nt = blockDim.x;
  const int Lraw = tgt_len[b];
  const bool bad_len = Lraw < 1 || Lraw > max_tgt;               // never computed: `targets` holds max_tgt labels per row
  const int Tb = max(min(in_len[b], T), 0), L = bad_len ? 0 : Lraw, S = 2 * L + 1;
  const float* lpb = lp + (int64_t)b * T * ld;
  const int64_t* tg = targets + (int64_t)b * ldt;
  uint8_t* bpb = ws + (int64_t)b * T * row_bytes;
  int32_t* ft = frame_token + (int64_t)b * T;
  int32_t* sp = spans + (int64_t)b * max_tgt * 2;
  float* ll = label_logp + (int64_t)b * max_tgt;
  const int s0 = i * R, j0 = s0 >> 1;
  const bool live = s0 < S;

  // the strip's labels and whether the step s-2 -> s is allowed, as in the loss
  uint32_t lab[H];                                               // unsigned: a 32-bit offset beside the frame's uniform row pointer
  bool skp[H];
  bool bad = false;
  int before = (j0 >= 1 && j0 - 1 < L) ? (int)tg[j0 - 1] : blank;
#pragma unroll
  for (int m = 0; m < H; ++m) {
    const int j = j0 + m;
    const bool lv = j < L;
    const int c = lv ? (int)tg[j] : blank;
    bad |= lv && (c < 0 || c >= V);
    skp[m] = lv && j >= 1 && c != blank && c != before;
    lab[m] = (uint32_t)c;
    before = c;
  }

  for (int e = i; e < max_tgt; e += nt) { sp[2 * e] = -1; sp[2 * e + 1] = -1; ll[e] = 0.f; }
  // a bad length, a label outside [0, V) (its gather would leave the row) or no frames: infeasible, nothing of it is computed
  if (__syncthreads_or(bad_len || bad || Tb == 0)) {
    for (int t = i; t < T; t += nt) ft[t] = -1;
    if (i == 0) { score[b] = NEG_INF; bounds[2 * b] = -1; bounds[2 * b + 1] = -1; }
    return;
  }
  for (int t = Tb + i; t < T; t += nt) ft[t] = -1;

  auto store_bp = [&](int t, uint32_t code) {
    if (R == 4) bpb[(int64_t)t * row_bytes + i] = (uint8_t)code;
    else ((uint16_t*)(bpb + (int64_t)t * row_bytes))[i] = (uint16_t)code;
  };

  // ---------------- best-path scores, frame by frame
  float p[R];
#pragma unroll
  for (int k = 0; k < R; ++k) p[k] = NEG_INF;
  if (i == 0) {
    p[0] = lpb[blank];
    p[1] = lpb[lab[0]];
    edge[0][0] = NEG_INF;
    edge[1][0] = NEG_INF;
    store_bp(0, 0xF);                                             // states 0 and 1: the path starts here
  }
  // No other thread stores a code for frame 0, and threads without a live state store none at all: the trace copies such workspace
  // words to LDS as they are, but it extracts only the bits of states on the path, and t == 0 ends the walk whatever row 0 holds.
  edge[0][i + 1] = p[R - 1];

  // the end candidate lives with the owner of state 2L
  const int i_end = (2 * L) / R, k_end = (2 * L) % R;
  float best = NEG_INF;
  int best_t = -1, best_s = -1;
  auto consider = [&](int t, float l1) {                          // frame t's end candidates from p = v_t and l1 = v_t(s0 - 1)
    float v2 = p[0], v1 = l1;
#pragma unroll
    for (int k = 2; k < R; k += 2) {                              // selects: an if becomes p[k_end], and p leaves the registers
      v2 = k == k_end ? p[k] : v2;
      v1 = k == k_end ? p[k - 1] : v1;
    }
    const float tail = t < Tb - 1 ? (float)(Tb - 1 - t) * skip_logp : 0.f;
    const float e2 = v2 + tail, e1 = v1 + tail;
    if (e2 > best) { best = e2; best_t = t; best_s = 2 * L; }     // earlier frames keep a tie, 2L before 2L-1
    if (e1 > best) { best = e1; best_t = t; best_s = 2 * L - 1; }
  };

  const bool vstart = free_start && i == 0;
  CsGather<R, PF> xa, xb;
  auto gather = [&](CsGather<R, PF>& x, int t0) {
#pragma unroll
    for (int f = 0; f < PF; ++f) {
      const bool ok = live && t0 + f < Tb;
      const float* row = lpb + (int64_t)(t0 + f) * ld;
      x.b[f] = ok ? row[blank] : 0.f;
#pragma unroll
      for (int m = 0; m < H; ++m) x.l[f][m] = ok ? row[lab[m]] : 0.f;
    }
  };
  auto frames = [&](const CsGather<R, PF>& x, int t0) {
#pragma unroll
    for (int f = 0; f < PF; ++f) {
      const int t = t0 + f;
      if (t >= Tb) break;                                         // Tb is uniform over the workgroup
      __syncthreads();
      const float l1 = edge[(t - 1) & 1][i];
      if (free_end && i == i_end) consider(t - 1, l1);
      const float vs = (float)t * skip_logp;
      float q[R];
      uint32_t code = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        float m = p[k];
        uint32_t c = 0;                                           // a later candidate wins only if strictly greater
        const float a1 = k ? p[k - 1] : l1;
        if (a1 > m) { m = a1; c = 1; }
        if (k & 1) {
          const float a2 = k >= 2 ? p[k - 2] : l1;
          if (skp[k >> 1] && a2 > m) { m = a2; c = 2; }
        }
        if (k < 2 && vstart && vs > m) { m = vs; c = 3; }         // the virtual start: t skipped frames
        q[k] = s0 + k < S ? m + ((k & 1) ? x.l[f][k >> 1] : x.b[f]) : NEG_INF;
        code |= c << (2 * k);
      }
#pragma unroll
      for (int k = 0; k < R; ++k) p[k] = q[k];
      edge[t & 1][i + 1] = p[R - 1];
      if (live) store_bp(t, code);
    }
  };
  gather(xa, 1);
  for (int t0 = 1; t0 < Tb; t0 += 2 * PF) {
    gather(xb, t0 + PF);
    frames(xa, t0);
    gather(xa, t0 + 2 * PF);
    frames(xb, t0 + PF);
  }
  __syncthreads();
  if (i == i_end) {
    consider(Tb - 1, edge[(Tb - 1) & 1][i]);
    s_best = best;
    s_cur[0] = best_t;
    s_cur[1] = best_s;
    score[b] = best;
  }
  __syncthreads();                                                // also: the back-pointers are visible to the whole workgroup
  if (!(s_best > NEG_INF)) {                                      // no path of finite score
    for (int t = i; t < Tb; t += nt) ft[t] = -1;
    if (i == 0) { bounds[2 * b] = -1; bounds[2 * b + 1] = -1; }
    return;
  }

  // ---------------- back-trace, a block of CS_TB frames per round: the frame -> state map goes to frame_token
  const int t_end = s_cur[0];
  const int row_words = (int)(row_bytes >> 2);
  int t_first;
  while (true) {
    const int ct = s_cur[0], cs = s_cur[1];
    const int wlo = max(cs - 2 * CS_TB, 0) >> 4;
    if (i < CS_TB && ct - i >= 0) {
      const uint32_t* row = (const uint32_t*)(bpb + (int64_t)(ct - i) * row_bytes);
#pragma unroll
      for (int w = 0; w < CS_TW; ++w) tr[i][w] = row[min(wlo + w, row_words - 1)];
    }
    __syncthreads();
    if (i == 0) {
      int st = cs, n = 0, done = 0, first = 0;
      for (int l = 0; l < CS_TB; ++l) {
        const int t = ct - l;
        path[l] = st;
        n = l + 1;
        const int code = (tr[l][(st >> 4) - wlo] >> ((st & 15) * 2)) & 3;
        if (code == 3 || t == 0) { done = 1; first = t; break; }
        st -= code;
      }
      s_cur[0] = ct - CS_TB;
      s_cur[1] = st;
      s_cur[2] = done;
      s_cur[3] = first;
      s_cur[4] = n;
    }
    __syncthreads();
    if (i < s_cur[4]) ft[ct - i] = path[i];
    if (s_cur[2]) { t_first = s_cur[3]; break; }
  }
  __syncthreads();
  if (i == 0) { bounds[2 * b] = t_first; bounds[2 * b + 1] = t_end + 1; }

  // ---------------- frame -> state map -> spans, tokens, per-label sums; the frames the path leaves out
  for (int t = t_first + i; t <= t_end; t += nt) {
    const int st = ft[t];
    if (st & 1) {
      if (t == t_first || ft[t - 1] != st) sp[2 * (st >> 1)] = t;
      if (t == t_end || ft[t + 1] != st) sp[2 * (st >> 1) + 1] = t + 1;
    }
  }
  __syncthreads();
  for (int t = t_first + i; t <= t_end; t += nt) {
    const int st = ft[t];
    ft[t] = (st & 1) ? (int)tg[st >> 1] : blank;
  }
  for (int t = i; t < t_first; t += nt) ft[t] = -1;
  for (int t = t_end + 1 + i; t < Tb; t += nt) ft[t] = -1;
  for (int j = i; j < L; j += nt) {
    const int t0 = sp[2 * j], t1 = sp[2 * j + 1];
    const float* col = lpb + (int)tg[j];
    float acc = 0.f;
    int t = t0;
    for (; t + 8 <= t1; t += 8) {                                 // the loads of 8 frames at once, the adds in ascending t
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = col[(int64_t)(t + u) * ld];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += x[u];
    }
    for (; t < t1; ++t) acc += col[(int64_t)t * ld];
    ll[j] = acc;
  }
}

extern "C" int64_t otr_ctc_segment_workspace_bytes(int32_t B, int32_t T, int32_t max_tgt) {
  if (B < 1 || T < 1 || T > CS_MAX_T || max_tgt < 1 || max_tgt > CS_MAX_TGT) return -1;
  return (int64_t)B * T * cs_row_bytes(max_tgt);
}

extern "C" int32_t otr_ctc_segment(const float* log_probs, int64_t ld, const int64_t* targets, int64_t ldt, const int32_t* in_len,
                                   const int32_t* tgt_len, int32_t B, int32_t T, int32_t V, int32_t max_tgt, int32_t blank,
                                   int32_t free_start, int32_t free_end, float skip_logp, void* workspace, int64_t ws_bytes,
                                   int32_t* frame_token, int32_t* spans, float* label_logp, float* score, int32_t* bounds,
                                   void* stream) {
  OTR_REQUIRE(log_probs && targets && in_len && tgt_len && workspace && frame_token && spans && label_logp && score && bounds,
              "ctc_segment: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1 && T <= CS_MAX_T && V > 1, "ctc_segment: bad shape B=%d T=%d V=%d (T <= %d)", B, T, V, CS_MAX_T);
  OTR_REQUIRE(max_tgt >= 1 && max_tgt <= CS_MAX_TGT, "ctc_segment: max_tgt=%d must be in [1, %d]", max_tgt, CS_MAX_TGT);
  OTR_REQUIRE(ld >= V && ldt >= max_tgt, "ctc_segment: ld=%lld must be >= V=%d and ldt=%lld >= max_tgt=%d", (long long)ld, V,
              (long long)ldt, max_tgt);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_segment: blank=%d must be in [0, V=%d)", blank, V);
  OTR_REQUIRE((free_start == 0 || free_start == 1) && (free_end == 0 || free_end == 1),
              "ctc_segment: free_start=%d and free_end=%d must be 0 or 1", free_start, free_end);
  OTR_REQUIRE(skip_logp <= 0.f && skip_logp >= -3.402823466e+38f, "ctc_segment: skip_logp=%g must be finite and <= 0",
              (double)skip_logp);
  OTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "ctc_segment: workspace must be 8-byte aligned");
  const int64_t need = otr_ctc_segment_workspace_bytes(B, T, max_tgt);
  OTR_REQUIRE(ws_bytes >= need, "ctc_segment: workspace of %lld bytes, %lld needed (otr_ctc_segment_workspace_bytes)",
              (long long)ws_bytes, (long long)need);
  const int nt = cs_threads(max_tgt);
  const int64_t row_bytes = cs_row_bytes(max_tgt);
  hipStream_t s = (hipStream_t)stream;
#define CS_LAUNCH(R, PF, NT)                                                                                                       \
  hipLaunchKernelGGL((ctc_segment_kernel<R, PF, NT>), dim3(B), dim3(nt), 0, s, log_probs, ld, targets, ldt, in_len, tgt_len, T, V,  \
                     max_tgt, blank, free_start, free_end, skip_logp, (uint8_t*)workspace, row_bytes, frame_token, spans,          \
                     label_logp, score, bounds)
  // the prefetch depth is what the registers of the workgroup's size leave: 512 per thread up to 256 threads, 128 at 1024 (no spills)
  if (nt <= 256) CS_LAUNCH(4, 16, 256);
  else if (cs_strip(max_tgt) == 4) CS_LAUNCH(4, 6, CS_NT);
  else CS_LAUNCH(8, 3, CS_NT);
#undef CS_LAUNCH
  return otr_check_launch("ctc_segment");
}
