// The transducer's beam search ("modified beam search": frame-synchronous, at most one symbol per frame, identical hypotheses merged
// before pruning): the three per-frame kernels.  include/otrans_hip.h states the semantics.  f32 in both builds; the 16-bit build
// parameter only names the type of the joint's operand twin.  Rows are R = B * W; slot r belongs to utterance r / W.  No atomics.
//  * beam_joint:   a workgroup per slot: z[r] = tanh(pe[r / W, t] + pg[r]) with its 16-bit twin, zeros for a slot that is dead or
//                  whose utterance has ended; 16-byte accesses.
//  * beam_select:  a workgroup per utterance, a WAVE per slot (64 W threads).
//                  (a) the slot's wave: max and sum-exp over V (16-byte loads behind the row's own alignment peel, as rnnt_rows does),
//                      then its W best non-blank logits, lowest index on ties: W sweeps of the row, sweep k taking the best element
//                      that comes after pick k - 1 in the order (value down, index up), so nothing picked has to be remembered;
//                  (b) the slot's wave looks for the one slot j whose history is its own minus the last token (a wave-wide compare of
//                      the two histories), adds s_j + lp_j[k] to its stay and strikes (j, k) from j's list if it is there;
//                  (c) a thread per candidate (W stays, then W lists of W extensions: the candidate's index IS the tie order) counts
//                      the candidates that beat it; rank < W takes output slot `rank`;
//                  (d) the output slot's wave copies the parent's history into the other half and appends the new token.
//  * beam_gather:  a workgroup per (row, item): dst[k][r] = src[k][(r / W) * W + parent[r]].
#include "common.h"

#ifndef NEG_INF
#define NEG_INF (-__builtin_huge_valf())
#endif

constexpr int RB_MAX = OTR_RNNT_BEAM_MAX;
constexpr int RB_CAND = RB_MAX * (RB_MAX + 1);
constexpr int RB_ITEMS = 16;
constexpr int RB_NONE = 0x7fffffff;

// ---------------------------------------------------------------- joint
__global__ __launch_bounds__(256) void rnnt_beam_joint_kernel(const float* pe, const float* pg, const float* score, const int32_t* enc_len, int W,
                                                              int T, int t, int J, float* z, bf16_t* z16) {
  const int r = blockIdx.x, b = r / W;
  const int Tb = min(max(enc_len[b], 0), T);
  const bool live = t < Tb && score[r] > NEG_INF;
  for (int q = threadIdx.x; q < (J >> 2); q += 256) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 a = *reinterpret_cast<const float4*>(pe + ((int64_t)b * T + t) * J + 4 * q);
      const float4 g = *reinterpret_cast<const float4*>(pg + (int64_t)r * J + 4 * q);
      o = make_float4(tanhf(a.x + g.x), tanhf(a.y + g.y), tanhf(a.z + g.z), tanhf(a.w + g.w));
    }
    *reinterpret_cast<float4*>(z + (int64_t)r * J + 4 * q) = o;
    if (z16) *reinterpret_cast<uint2*>(z16 + (int64_t)r * J + 4 * q) = make_uint2(pack2h(o.x, o.y), pack2h(o.z, o.w));
  }
}

// ---------------------------------------------------------------- select: the row sweeps
struct RbRun { float m, s; };
__device__ __forceinline__ void rb_take(RbRun& r, float x) {
  if (x > r.m) {
    r.s = r.s * expf(r.m - x) + 1.f;
    r.m = x;
  } else if (x > NEG_INF) {
    r.s += expf(x - r.m);
  }
}
__device__ __forceinline__ void rb_take4(RbRun& r, const float4& q) {
  const float mq = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  if (mq > r.m) {
    r.s *= expf(r.m - mq);
    r.m = mq;
  }
  if (r.m > NEG_INF) r.s += (expf(q.x - r.m) + expf(q.y - r.m)) + (expf(q.z - r.m) + expf(q.w - r.m));
}
// floats in front of the first 16-byte boundary of a row (the row's own peel), at most n
__device__ __forceinline__ int rb_head(const float* x, int n) { return min((int)((4u - (uint32_t)(((uintptr_t)x >> 2) & 3u)) & 3u), n); }

__device__ __forceinline__ void rb_row(const float* x, int V, int lane, float& M, float& S) {
  RbRun r{NEG_INF, 0.f};
  const int head = rb_head(x, V);
  if (lane < head) rb_take(r, x[lane]);
  const float* xa = x + head;
  const int nq = (V - head) >> 2;
  int q = lane;
  for (; q + 192 < nq; q += 256) {                    // four loads in flight per lane
    const float4 a = *reinterpret_cast<const float4*>(xa + 4 * q);
    const float4 b = *reinterpret_cast<const float4*>(xa + 4 * (q + 64));
    const float4 c = *reinterpret_cast<const float4*>(xa + 4 * (q + 128));
    const float4 d = *reinterpret_cast<const float4*>(xa + 4 * (q + 192));
    rb_take4(r, a); rb_take4(r, b); rb_take4(r, c); rb_take4(r, d);
  }
  for (; q < nq; q += 64) rb_take4(r, *reinterpret_cast<const float4*>(xa + 4 * q));
  for (int v = head + 4 * nq + lane; v < V; v += 64) rb_take(r, x[v]);
  M = wave_max(r.m);
  S = wave_sum(r.m > NEG_INF ? r.s * expf(r.m - M) : 0.f);
}

// the order of a slot's extensions: value down, index up
struct RbPick { float v; int i; };
__device__ __forceinline__ bool rb_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
__device__ __forceinline__ void rb_offer(RbPick& best, const RbPick& prev, float xv, int idx, int blank) {
  if (idx != blank && rb_before(prev.v, prev.i, xv, idx) && rb_before(xv, idx, best.v, best.i)) {
    best.v = xv;
    best.i = idx;
  }
}
// the best non-blank element of the row that comes after `prev`; i == RB_NONE when there is none
__device__ __forceinline__ RbPick rb_next(const float* x, int V, int lane, const RbPick& prev, int blank) {
  RbPick best{NEG_INF, RB_NONE};
  const int head = rb_head(x, V);
  if (lane < head) rb_offer(best, prev, x[lane], lane, blank);
  const float* xa = x + head;
  const int nq = (V - head) >> 2;
  for (int q = lane; q < nq; q += 64) {
    const float4 a = *reinterpret_cast<const float4*>(xa + 4 * q);
    const int v = head + 4 * q;
    rb_offer(best, prev, a.x, v, blank);
    rb_offer(best, prev, a.y, v + 1, blank);
    rb_offer(best, prev, a.z, v + 2, blank);
    rb_offer(best, prev, a.w, v + 3, blank);
  }
  for (int v = head + 4 * nq + lane; v < V; v += 64) rb_offer(best, prev, x[v], v, blank);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best.v, o);
    const int oi = __shfl_xor(best.i, o);
    if (rb_before(ov, oi, best.v, best.i)) {
      best.v = ov;
      best.i = oi;
    }
  }
  return best;
}

__device__ __forceinline__ float rb_lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + log1pf(expf(-fabsf(a - b)));
}

// ---------------------------------------------------------------- select
__global__ __launch_bounds__(64 * RB_MAX) void rnnt_beam_select_kernel(const float* logits, int64_t ld, const int32_t* enc_len, int W, int T, int t,
                                                                       int V, int blank, int max_len, const float* score_in, const int32_t* n_in,
                                                                       const int64_t* tokens_in, const int32_t* frames_in, float* score_out,
                                                                       int32_t* n_out, int64_t* tokens_out, int32_t* frames_out, int32_t* parent,
                                                                       int64_t* step_tok, int32_t* emit) {
  __shared__ float s_sc[RB_MAX];                      // the live slots' scores (-inf: dead), lengths and log-sum-exp
  __shared__ int s_n[RB_MAX];
  __shared__ float s_lse[RB_MAX];
  __shared__ float c_s[RB_CAND];                      // candidates: [0, W) the stays, W + i * W + k extension k of slot i; -inf: none
  __shared__ int c_tok[RB_CAND];
  __shared__ int s_sel[RB_MAX];                       // output slot -> candidate
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = (int64_t)b * W, r = r0 + w;
  const int Tb = min(max(enc_len[b], 0), T);
  const float s_i = score_in[r];
  const int n_i = min(max(n_in[r], 0), max_len);
  const int64_t* tk_i = tokens_in + r * max_len;
  if (t >= Tb) {                                      // the utterance has ended: carried over unchanged into the other half
    const int32_t* fr_i = frames_in + r * max_len;
    for (int p = lane; p < n_i; p += 64) {
      tokens_out[r * max_len + p] = tk_i[p];
      frames_out[r * max_len + p] = fr_i[p];
    }
    if (lane == 0) {
      score_out[r] = s_i;
      n_out[r] = n_i;
      parent[r] = w;
      step_tok[r] = blank;
      emit[r] = 0;
    }
    return;
  }
  const bool live = s_i > NEG_INF;
  const int nc = W * (W + 1);
  for (int c = tid; c < nc; c += 64 * W) {
    c_s[c] = NEG_INF;
    c_tok[c] = -1;
  }
  if (lane == 0) {
    s_sc[w] = live ? s_i : NEG_INF;
    s_n[w] = n_i;
    s_lse[w] = 0.f;
    s_sel[w] = -1;
  }
  __syncthreads();
  // (a) log-sum-exp, the stay and the slot's W best extensions
  const float* x = logits + r * ld;
  if (live) {
    float M, S;
    rb_row(x, V, lane, M, S);
    const float lse = M + logf(S);
    if (lane == 0) {
      s_lse[w] = lse;
      c_s[w] = s_i + (x[blank] - lse);
      c_tok[w] = blank;
    }
    if (n_i < max_len) {                              // a slot at max_len offers only its stay
      RbPick prev{__builtin_huge_valf(), -1};
      for (int k = 0; k < W; ++k) {
        const RbPick best = rb_next(x, V, lane, prev, blank);
        if (best.i == RB_NONE) break;                 // fewer than W non-blank units
        if (lane == 0) {
          c_s[W + w * W + k] = s_i + (best.v - lse);
          c_tok[W + w * W + k] = best.i;
        }
        prev = best;
      }
    }
  }
  __syncthreads();
  // (b) the merge: the stay of i joins the extension (j, k) with y_i == y_j + [k]; live hypotheses are distinct, so there is one j at most
  if (live && n_i >= 1) {
    for (int j = 0; j < W; ++j) {
      const float s_j = s_sc[j];
      const int n_j = s_n[j];
      if (j == w || !(s_j > NEG_INF) || n_j + 1 != n_i) continue;
      const int64_t* tk_j = tokens_in + (r0 + j) * max_len;
      bool eq = true;
      for (int p = lane; p < n_j; p += 64) eq = eq && tk_i[p] == tk_j[p];
      if (!__all(eq)) continue;
      const int64_t k = tk_i[n_j];
      if (k >= 0 && k < V && k != blank && lane == 0) {
        const float partner = s_j + (logits[(r0 + j) * ld + k] - s_lse[j]);   // read from row j whether or not k is among j's W best
        c_s[w] = rb_lae(c_s[w], partner);
        for (int kk = 0; kk < W; ++kk)
          if (c_tok[W + j * W + kk] == (int)k) c_s[W + j * W + kk] = NEG_INF;   // the candidate that was merged away
      }
      break;
    }
  }
  __syncthreads();
  // (c) the W best candidates: higher score first; equal scores in the order of the candidate index, which is the tie rule (a stay
  //     before an extension, the lower parent, the lower token: a slot's list holds equal LOGITS by ascending token).  One corner is
  //     not the rule to the letter: two different logits of one slot whose f32 scores s_i + (x - lse) round to the same number keep
  //     the order of their logits, not of their tokens.  In exact arithmetic they do not tie at all, so this is the order the rule's
  //     own premise gives; a float64 restatement that rounds nothing never meets the case.
  if (tid < nc) {
    const float s = c_s[tid];
    if (s > NEG_INF) {
      int rank = 0;
      for (int c = 0; c < nc; ++c) {
        const float o = c_s[c];
        rank += (o > s || (o == s && c < tid)) ? 1 : 0;
      }
      if (rank < W) s_sel[rank] = tid;
    }
  }
  __syncthreads();
  // (d) output slot w, in rank order
  const int c = s_sel[w];
  if (c < 0) {                                        // fewer candidates than slots: dead
    if (lane == 0) {
      score_out[r] = NEG_INF;
      n_out[r] = 0;
      parent[r] = w;
      step_tok[r] = blank;
      emit[r] = 0;
    }
    return;
  }
  const bool ext = c >= W;
  const int par = ext ? (c - W) / W : c;
  const int np = s_n[par];
  const int64_t* tk_p = tokens_in + (r0 + par) * max_len;
  const int32_t* fr_p = frames_in + (r0 + par) * max_len;
  for (int p = lane; p < np; p += 64) {
    tokens_out[r * max_len + p] = tk_p[p];
    frames_out[r * max_len + p] = fr_p[p];
  }
  if (lane == 0) {
    const int tok = c_tok[c];
    if (ext) {                                        // np < max_len: the slot offered extensions
      tokens_out[r * max_len + np] = tok;
      frames_out[r * max_len + np] = t;
    }
    score_out[r] = c_s[c];
    n_out[r] = np + (ext ? 1 : 0);
    parent[r] = par;
    step_tok[r] = ext ? tok : blank;
    emit[r] = ext ? 1 : 0;
  }
}

// ---------------------------------------------------------------- gather
struct RbGather {
  const void* src[RB_ITEMS];
  void* dst[RB_ITEMS];
  int32_t words[RB_ITEMS];                            // 4-byte words per row
};
__global__ __launch_bounds__(256) void rnnt_beam_gather_kernel(const int32_t* parent, int W, RbGather g) {
  const int r = blockIdx.x, k = blockIdx.y;
  const int p = min(max(parent[r], 0), W - 1);        // never an index outside the utterance's slots
  const int n = g.words[k];
  const uint32_t* s = (const uint32_t*)g.src[k] + ((int64_t)(r / W) * W + p) * n;
  uint32_t* d = (uint32_t*)g.dst[k] + (int64_t)r * n;
  if ((n & 3) == 0 && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
    for (int i = threadIdx.x; i < (n >> 2); i += 256) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
  } else {
    for (int i = threadIdx.x; i < n; i += 256) d[i] = s[i];
  }
}

// ---------------------------------------------------------------- entries
static bool rnnt_beam_rows_ok(int64_t B, int64_t W) { return B >= 1 && W >= 1 && W <= OTR_RNNT_BEAM_MAX && B * W <= 65535; }

extern "C" int32_t otr_rnnt_beam_joint(const float* pe, const float* pg, const float* score, const int32_t* enc_len, int32_t B, int32_t W,
                                       int32_t T, int32_t t, int32_t J, float* z, void* z16, void* stream) {
  OTR_REQUIRE(rnnt_beam_rows_ok(B, W), "rnnt_beam_joint: B=%d, W=%d: 1 <= W <= %d and B * W <= 65535 rows expected", B, W, OTR_RNNT_BEAM_MAX);
  OTR_REQUIRE(T >= 1 && t >= 0 && t < T, "rnnt_beam_joint: frame t=%d outside [0, T=%d)", t, T);
  OTR_REQUIRE(J >= 4 && J % 4 == 0, "rnnt_beam_joint: J=%d must be a positive multiple of 4", J);
  OTR_REQUIRE(pe && pg && score && enc_len && z, "rnnt_beam_joint: null pointer");
  OTR_REQUIRE(((uintptr_t)pe | (uintptr_t)pg | (uintptr_t)z) % 16 == 0 && (uintptr_t)z16 % 8 == 0,
              "rnnt_beam_joint: pe, pg, z must be 16-byte aligned");
  hipLaunchKernelGGL(rnnt_beam_joint_kernel, dim3((unsigned)(B * W)), dim3(256), 0, (hipStream_t)stream, pe, pg, score, enc_len, W, T, t, J, z,
                     (bf16_t*)z16);
  return otr_check_launch("rnnt_beam_joint");
}

extern "C" int32_t otr_rnnt_beam_select(const float* logits, int64_t ld, const int32_t* enc_len, int32_t B, int32_t W, int32_t T, int32_t t,
                                        int32_t V, int32_t blank, int32_t max_len, const float* score_in, const int32_t* n_in,
                                        const int64_t* tokens_in, const int32_t* frames_in, float* score_out, int32_t* n_out,
                                        int64_t* tokens_out, int32_t* frames_out, int32_t* parent, int64_t* step_tok, int32_t* emit,
                                        void* stream) {
  OTR_REQUIRE(rnnt_beam_rows_ok(B, W), "rnnt_beam_select: B=%d, W=%d: 1 <= W <= %d and B * W <= 65535 rows expected", B, W, OTR_RNNT_BEAM_MAX);
  OTR_REQUIRE(T >= 1 && t >= 0 && t < T, "rnnt_beam_select: frame t=%d outside [0, T=%d)", t, T);
  OTR_REQUIRE(V >= 2 && ld >= V && blank >= 0 && blank < V, "rnnt_beam_select: V=%d >= 2, ld=%lld >= V, blank=%d in [0, V) expected", V,
              (long long)ld, blank);
  OTR_REQUIRE(max_len >= 1 && max_len <= OTR_RNNT_BEAM_MAX_LEN, "rnnt_beam_select: max_len=%d outside [1, %d]", max_len, OTR_RNNT_BEAM_MAX_LEN);
  OTR_REQUIRE(logits && enc_len && score_in && n_in && tokens_in && frames_in && score_out && n_out && tokens_out && frames_out && parent &&
                  step_tok && emit,
              "rnnt_beam_select: null pointer");
  OTR_REQUIRE(score_in != score_out && n_in != n_out && tokens_in != tokens_out && frames_in != frames_out,
              "rnnt_beam_select: the beam is double-buffered: the in and out halves must differ");
  hipLaunchKernelGGL(rnnt_beam_select_kernel, dim3((unsigned)B), dim3(64 * W), 0, (hipStream_t)stream, logits, ld, enc_len, W, T, t, V, blank,
                     max_len, score_in, n_in, tokens_in, frames_in, score_out, n_out, tokens_out, frames_out, parent, step_tok, emit);
  return otr_check_launch("rnnt_beam_select");
}

extern "C" int32_t otr_rnnt_beam_gather(const int32_t* parent, const void* const* src, void* const* dst, const int32_t* row_bytes,
                                        int32_t n_items, int32_t B, int32_t W, void* stream) {
  OTR_REQUIRE(rnnt_beam_rows_ok(B, W), "rnnt_beam_gather: B=%d, W=%d: 1 <= W <= %d and B * W <= 65535 rows expected", B, W, OTR_RNNT_BEAM_MAX);
  OTR_REQUIRE(n_items >= 1 && n_items <= RB_ITEMS, "rnnt_beam_gather: n_items=%d (1 .. %d) not supported", n_items, RB_ITEMS);
  OTR_REQUIRE(parent && src && dst && row_bytes, "rnnt_beam_gather: null pointer");
  RbGather g;
  for (int k = 0; k < RB_ITEMS; ++k) {
    const int j = k < n_items ? k : 0;
    OTR_REQUIRE(src[j] && dst[j] && src[j] != dst[j] && row_bytes[j] > 0 && row_bytes[j] % 4 == 0 &&
                    ((uintptr_t)src[j] | (uintptr_t)dst[j]) % 4 == 0,
                "rnnt_beam_gather: item %d needs distinct 4-byte aligned buffers and a row of a positive multiple of 4 bytes", j);
    g.src[k] = src[j];
    g.dst[k] = dst[j];
    g.words[k] = row_bytes[j] / 4;
  }
  hipLaunchKernelGGL(rnnt_beam_gather_kernel, dim3((unsigned)(B * W), n_items), dim3(256), 0, (hipStream_t)stream, parent, W, g);
  return otr_check_launch("rnnt_beam_gather");
}
