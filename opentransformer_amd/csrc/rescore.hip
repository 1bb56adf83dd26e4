// Attention rescoring of the CTC n-best (SpeechToTextRecognizer rescore=True): the glue between the CTC prefix beam search
// (csrc/ctcbeam.hip) and ONE teacher-forced pass of the attention decoder (and the LM) over all B x W hypotheses.  include/otrans_hip.h
// states the semantics.  f32 in both builds.
//  * rescore_pack:    the search's tokens [B, W, T] -> decoder input [BOS, h, filler], targets [h, EOS, -1 ...] and the row count
//                     len + 1 of every hypothesis (0: dead or too long).  One thread per (hypothesis, position).
//  * rescore_score:   per hypothesis the sum over its first n_rows positions of logit[target] - logsumexp(row).  One workgroup per
//                     (hypothesis, logits tensor), one WAVE per row: the row is read once (16-byte loads where its address allows) into
//                     an online max / sum, rows at or past n_rows are never touched, no log-softmax tensor is written.  Wave w adds up
//                     rows w, w + 4, ... in order and thread 0 adds the four partials in order: the same sum on every run.
//  * rescore_select:  one workgroup per utterance: total = (1 - lambda) att + lambda ctc + mu lm (+ add), the length penalty, the rank of each
//                     of the W <= 32 entries by counting (ties -> lower CTC rank, -inf last in CTC order), then the n-best rows leave.
#include "common.h"
#include "rowlse.h"      // NEG_INF, rs_row: one wave's online logsumexp of a row (shared with mwer.hip)

constexpr int RS_MAXW = 32;       // the search's beam limit
constexpr int RS_MAXV = 8192;     // the search's vocabulary limit

// ---------------------------------------------------------------- pack
__global__ __launch_bounds__(256) void rescore_pack_kernel(const int64_t* tokens, const int32_t* out_len, const float* scores, int64_t nh, int T,
                                                           int max_len, int V, int bos, int eos, int64_t* ys_in, int64_t* ys_out,
                                                           int32_t* n_rows) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nh * max_len) return;
  const int64_t h = idx / max_len;
  const int l = (int)(idx - h * max_len);
  const int n = out_len[h];
  const bool live = scores[h] > NEG_INF && n >= 0 && n <= T && n + 1 <= max_len;
  const int64_t* tok = tokens + h * T;
  int64_t in = eos, out = -1;                         // behind the hypothesis: any valid id (the causal mask keeps it from mattering) / no target
  if (live) {
    if (l >= 1 && l <= n) in = min(max(tok[l - 1], (int64_t)0), (int64_t)(V - 1));
    out = l < n ? tok[l] : (l == n ? (int64_t)eos : (int64_t)-1);
  }
  if (l == 0) {
    in = bos;
    n_rows[h] = live ? n + 1 : 0;
  }
  ys_in[idx] = in;
  ys_out[idx] = out;
}

extern "C" int32_t otr_rescore_pack(const int64_t* tokens, const int32_t* out_len, const float* scores, int64_t n_hyp, int32_t T,
                                    int32_t max_len, int32_t V, int32_t bos, int32_t eos, int64_t* ys_in, int64_t* ys_out, int32_t* n_rows,
                                    void* stream) {
  OTR_REQUIRE(tokens && out_len && scores && ys_in && ys_out && n_rows, "rescore_pack: null pointer");
  OTR_REQUIRE(n_hyp > 0 && T > 0 && max_len >= 1 && n_hyp * (int64_t)max_len < (1ll << 31), "rescore_pack: bad shape n_hyp=%lld T=%d max_len=%d",
              (long long)n_hyp, T, max_len);
  OTR_REQUIRE(V >= 1 && V <= RS_MAXV && bos >= 0 && bos < V && eos >= 0 && eos < V, "rescore_pack: V=%d must be in [1, %d], BOS / EOS inside it", V,
              RS_MAXV);
  const int64_t n = n_hyp * max_len;
  hipLaunchKernelGGL(rescore_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tokens, out_len, scores, n_hyp, T,
                     max_len, V, bos, eos, ys_in, ys_out, n_rows);
  return otr_check_launch("rescore_pack");
}

// ---------------------------------------------------------------- score
__global__ __launch_bounds__(256) void rescore_score_kernel(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm,
                                                            const int64_t* ys_out, int64_t ldt, const int32_t* n_rows, int64_t nh, int max_len,
                                                            int V, float* att, float* lm) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool second = (int64_t)blockIdx.x >= nh;      // the LM's logits: the second half of the grid
  const int64_t h = (int64_t)blockIdx.x - (second ? nh : 0);
  const float* base = second ? lm_logits : logits;
  const int64_t ldx = second ? ld_lm : ld;
  float* out = second ? lm : att;
  const int n = min(max(n_rows[h], 0), max_len);
  if (n == 0) {
    if (tid == 0) out[h] = NEG_INF;
    return;
  }
  const bool vec = ((uintptr_t)base % 16 == 0) && (ldx % 4 == 0);      // every row starts on a 16-byte boundary
  float acc = 0.f;
  for (int l = wid; l < n; l += 4) {
    const float* x = base + (h * max_len + l) * ldx;
    float M, S;
    rs_row(x, V, vec, lane, M, S);
    const int64_t t = ys_out[h * ldt + l];
    if (t >= 0 && t < V) acc += x[t] - (M + __logf(S));
  }
  if (lane == 0) part[wid] = acc;
  __syncthreads();
  if (tid == 0) out[h] = ((part[0] + part[1]) + part[2]) + part[3];    // a wave without rows left 0
}

extern "C" int32_t otr_rescore_score(const float* logits, int64_t ld, const float* lm_logits, int64_t ld_lm, const int64_t* ys_out, int64_t ld_ys,
                                     const int32_t* n_rows, int64_t n_hyp, int32_t max_len, int32_t V, float* att_score, float* lm_score,
                                     void* stream) {
  OTR_REQUIRE(logits && ys_out && n_rows && att_score, "rescore_score: null pointer");
  OTR_REQUIRE(V >= 1 && V <= RS_MAXV && ld >= V, "rescore_score: V=%d must be in [1, %d], ld >= V", V, RS_MAXV);
  OTR_REQUIRE(!lm_logits || (ld_lm >= V && lm_score), "rescore_score: LM logits need ld_lm >= V and an output");
  OTR_REQUIRE(n_hyp > 0 && max_len >= 1 && ld_ys >= max_len && n_hyp < (1ll << 30), "rescore_score: bad shape n_hyp=%lld max_len=%d ld_ys=%lld",
              (long long)n_hyp, max_len, (long long)ld_ys);
  const unsigned grid = (unsigned)(lm_logits ? 2 * n_hyp : n_hyp);
  hipLaunchKernelGGL(rescore_score_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, lm_logits, ld_lm, ys_out, ld_ys, n_rows,
                     n_hyp, max_len, V, att_score, lm_score);
  return otr_check_launch("rescore_score");
}

// ---------------------------------------------------------------- select
__global__ __launch_bounds__(256) void rescore_select_kernel(const int64_t* tokens, const int32_t* out_len, const float* ctc, const int32_t* n_rows,
                                                             const float* att, const float* lm, const float* add, int W, int T, int nbest,
                                                             float lam, float mu, float penalty, float lamda, float* total, int32_t* perm, int64_t* nb_tokens,
                                                             int32_t* nb_len, float* nb_score) {
  __shared__ float s_tot[RS_MAXW];
  __shared__ int s_src[RS_MAXW];                      // rank -> CTC slot
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (tid < W) {
    const int64_t h = b * W + tid;
    float t = NEG_INF;
    if (n_rows[h] > 0) {
      t = (1.f - lam) * att[h] + lam * ctc[h];
      if (lm) t += mu * lm[h];
      if (add) t += add[h];                           // otr_rescore_select_add: a further term, inside the penalty's division
      if (penalty != 0.f) t /= powf((lamda + (float)(n_rows[h] - 1)) / (lamda + 1.f), penalty);
      if (!(t == t)) t = NEG_INF;                     // NaN ranks as -inf
    }
    s_tot[tid] = t;
    total[h] = t;
  }
  __syncthreads();
  if (tid < W) {
    const float t = s_tot[tid];
    int r = 0;
    for (int q = 0; q < W; ++q) r += s_tot[q] > t || (s_tot[q] == t && q < tid);
    s_src[r] = tid;
    perm[b * W + r] = tid;
    if (r < nbest) {
      nb_score[b * nbest + r] = t;
      nb_len[b * nbest + r] = out_len[b * W + tid];
    }
  }
  __syncthreads();
  for (int i = tid; i < nbest * T; i += 256) {
    const int r = i / T, j = i - r * T;
    nb_tokens[(b * nbest + r) * T + j] = tokens[(b * W + s_src[r]) * T + j];
  }
}

extern "C" int32_t otr_rescore_select_add(const int64_t* tokens, const int32_t* out_len, const float* ctc_score, const int32_t* n_rows,
                                          const float* att_score, const float* lm_score, const float* add_score, int32_t B, int32_t W,
                                          int32_t T, int32_t nbest, float ctc_weight, float lm_weight, float penalty, float lamda,
                                          float* total, int32_t* perm, int64_t* nbest_tokens, int32_t* nbest_len, float* nbest_score,
                                          void* stream) {
  OTR_REQUIRE(tokens && out_len && ctc_score && n_rows && att_score && total && perm && nbest_tokens && nbest_len && nbest_score,
              "rescore_select: null pointer");
  OTR_REQUIRE(B > 0 && T > 0, "rescore_select: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(W >= 1 && W <= RS_MAXW, "rescore_select: W=%d must be in [1, %d]", W, RS_MAXW);
  OTR_REQUIRE(nbest >= 1 && nbest <= W, "rescore_select: nbest=%d must be in [1, W=%d]", nbest, W);
  OTR_REQUIRE(ctc_weight >= 0.f && ctc_weight <= 1.f, "rescore_select: ctc_weight=%g must be in [0, 1]", (double)ctc_weight);
  OTR_REQUIRE(lm_weight == lm_weight && penalty == penalty && lamda + 1.f > 0.f, "rescore_select: bad lm_weight / penalty / lamda");
  hipLaunchKernelGGL(rescore_select_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, tokens, out_len, ctc_score, n_rows, att_score,
                     lm_score, add_score, W, T, nbest, ctc_weight, lm_weight, penalty, lamda, total, perm, nbest_tokens, nbest_len, nbest_score);
  return otr_check_launch("rescore_select");
}

extern "C" int32_t otr_rescore_select(const int64_t* tokens, const int32_t* out_len, const float* ctc_score, const int32_t* n_rows,
                                      const float* att_score, const float* lm_score, int32_t B, int32_t W, int32_t T, int32_t nbest,
                                      float ctc_weight, float lm_weight, float penalty, float lamda, float* total, int32_t* perm,
                                      int64_t* nbest_tokens, int32_t* nbest_len, float* nbest_score, void* stream) {
  return otr_rescore_select_add(tokens, out_len, ctc_score, n_rows, att_score, lm_score, nullptr, B, W, T, nbest, ctc_weight, lm_weight,
                                penalty, lamda, total, perm, nbest_tokens, nbest_len, nbest_score, stream);
}
