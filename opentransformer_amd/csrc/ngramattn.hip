// Backoff n-gram LM fusion for the attention, joint and two-pass decoders (SpeechToTextRecognizer ngram_lm=...).  ngram.h holds the
// table, the probe and the combine; include/otrans_hip.h states the semantics.  f32 in both builds.
//  * ngram_score_cands: the addend a(g, c) = alpha * ln P(c | context(g)) + (c == eos ? 0 : beta) of every pre-beam candidate of every
//                       hypothesis row, added into cand_score; optionally the top-`beam` of a row's K' totals in the prune's layout.
//                       A row owns 32 lanes, one per candidate.  What depends on the row alone -- the backoffs of its <= 4 context
//                       suffixes and the unigrams that say whether the context holds an OOV id, 7 keys -- is probed by lanes 0-6 of the
//                       row, one key each, next to that lane's own 5 n-gram keys, and handed round by shuffle.
//  * ngram_score_seqs:  alpha * (sum of ln P over the tokens of a hypothesis and its </s>) + beta * length.  One wave per hypothesis,
//                       one lane per position; lane sums, then the wave's butterfly: the same order on every run.
#include "ngram.h"

#define NEG_INF (-__builtin_huge_valf())

constexpr int NA_MAXK = 32;       // the pre-beam's K'
constexpr int NA_MAXBEAM = 16;    // the prune's limit
constexpr int NA_ROWS = 8;        // hypothesis rows per workgroup: 32 lanes each

__global__ __launch_bounds__(256) void ngram_score_cands_kernel(NgTable tb, int order, int V, const int64_t* preds, int64_t ldp, int t_host,
                                                                const int32_t* pos, const uint8_t* flags, const int32_t* cand_idx,
                                                                const float* cand_score, int64_t rows, int K, float alpha, float beta,
                                                                float oov_score, int eos, float* cand_out, float* cand_add, int beam,
                                                                float* k_score, int64_t* k_idx) {
  const int tid = threadIdx.x, lane = tid & 63, k = tid & 31, base = lane & 32;
  const int64_t row = (int64_t)blockIdx.x * NA_ROWS + (tid >> 5);
  const bool in_row = row < rows;
  const bool fin = in_row && flags && flags[row];
  const bool act = in_row && k < K;                     // this lane holds a candidate
  const bool score = act && !fin;
  int t = pos ? *pos + 1 : t_host;                      // prefix columns: <s> (by position) + t - 1 tokens
  t = min(max(t, 1), (int)min(ldp, (int64_t)0x7fffffff));
  const int L = min(t, order - 1);                      // ids of the context
  // the context packed newest id first; column 0 is <s> whatever it holds
  uint64_t cx = 0;
  bool bad_ctx = false;
  if (in_row && !fin) {
    for (int j = 0; j < L; ++j) {
      const int col = t - 1 - j;
      const int64_t id = col == 0 ? (int64_t)V : preds[row * ldp + col];
      bad_ctx |= id < 0 || id > V;
      cx |= (uint64_t)((uint32_t)id & 0xffffu) << (16 * j);
    }
  }
  const int c = act ? cand_idx[row * K + k] : 0;
  const float cs = act ? cand_score[row * K + k] : NEG_INF;
  const bool bad = bad_ctx || c < 0 || c > V;
  // keys 0 .. 4: the n-grams (newest j ids, c); key 5: this lane's share of the row's keys -- lanes 0-3 the context suffix of
  // k + 1 ids, lanes 4-6 the unigram of context id k - 3 (0 = the newest, whose unigram is suffix 1)
  constexpr int NP = NG_MAXN + 1;
  uint64_t klo[NP], khi[NP];
  float lp[NP], bo[NP];
  const uint64_t glo = (cx << 16) | (uint64_t)(uint32_t)c;
  const uint32_t ghi = (uint32_t)(cx >> 48);
#pragma unroll
  for (int j = 0; j < NG_MAXN; ++j) ng_key(glo, ghi, j + 1, klo[j], khi[j]);
  const bool is_suffix = k < NG_MAXN - 1;
  const bool row_want = in_row && !fin && !bad_ctx && (is_suffix ? k + 1 <= L : (k < 2 * NG_MAXN - 3 && k - 3 <= L - 1));
  if (is_suffix) ng_key(cx, 0u, k + 1, klo[NG_MAXN], khi[NG_MAXN]);
  else ng_key(cx >> (16 * ((k - 3) & 3)), 0u, 1, klo[NG_MAXN], khi[NG_MAXN]);
  uint32_t want = (score && !bad) ? (2u << L) - 1u : 0u;
  if (row_want) want |= 1u << NG_MAXN;
  const uint32_t found = ng_find<NP>(tb, klo, khi, want, lp, bo);
  // the row's part, through the wave: is every wanted context key there (suffix 1 and the older unigrams decide OOV; a longer
  // suffix that is not stored only adds no backoff), and the four backoffs
  const bool row_hit = (found >> NG_MAXN) & 1;
  const bool oov_lane = row_want && !row_hit && (k == 0 || !is_suffix);
  const uint64_t oov_mask = __ballot(oov_lane);
  const bool ctx_oov = ((uint32_t)(oov_mask >> base) & 0x7fu) != 0;
  const float my_bo = (row_want && row_hit && is_suffix) ? bo[NG_MAXN] : 0.f;
  float cbo[NG_MAXN - 1];
#pragma unroll
  for (int j = 0; j < NG_MAXN - 1; ++j) cbo[j] = __shfl(my_bo, base + j);
  float add = 0.f, out = cs;
  if (score) {
    float glp[NG_MAXN];
#pragma unroll
    for (int j = 0; j < NG_MAXN; ++j) glp[j] = lp[j];
    const float lnp = (bad || ctx_oov || !(found & 1u)) ? oov_score : ng_combine(found, glp, cbo, L);
    add = __fmul_rn(alpha, lnp);                        // alpha * ln P, then + beta: two roundings, as the contract states them
    if (c != eos) add = __fadd_rn(add, beta);
    out = cs == NEG_INF ? NEG_INF : __fadd_rn(cs, add);
  }
  if (act) {
    cand_out[row * K + k] = out;
    if (cand_add) cand_add[row * K + k] = add;
  }
  if (beam <= 0) return;                                // (uniform) no select
  // the rank of this lane's total among the row's K': by counting over the row's lanes (descending, ties -> lower token, then slot)
  const float v = (act && out == out) ? out : NEG_INF;  // NaN ranks as -inf
  int r = 0;
  for (int q = 0; q < K; ++q) {
    const float o = __shfl(v, base + q);
    const int oc = __shfl(c, base + q);
    r += o > v || (o == v && (oc < c || (oc == c && q < k)));
  }
  if (act && r < beam) {
    k_score[row * beam + r] = fin ? NEG_INF : v;        // a finished row: the prune masks its entries
    k_idx[row * beam + r] = fin ? (int64_t)eos : (int64_t)c;
  }
}

extern "C" int32_t otr_ngram_score_cands(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V,
                                         const int64_t* preds, int64_t ldp, int32_t t, const int32_t* pos, const uint8_t* flags,
                                         const int32_t* cand_idx, const float* cand_score, int64_t rows, int32_t K, float alpha, float beta,
                                         float oov_score, int32_t eos, float* cand_out, float* cand_add, int32_t beam, float* k_score,
                                         int64_t* k_idx, void* stream) {
  if (otr_ngram_check_table("ngram_score_cands", table, capacity, max_probe, order, V) < 0) return -1;
  OTR_REQUIRE(preds && cand_idx && cand_score && cand_out, "ngram_score_cands: null pointer");
  OTR_REQUIRE(K >= 1 && K <= NA_MAXK, "ngram_score_cands: K=%d must be in [1, %d]", K, NA_MAXK);
  OTR_REQUIRE(rows >= 0 && rows < (1ll << 31), "ngram_score_cands: bad rows");
  OTR_REQUIRE(ldp >= 1 && (pos || (t >= 1 && t <= ldp)), "ngram_score_cands: t=%d must be in [1, ldp=%lld]", t, (long long)ldp);
  OTR_REQUIRE(eos >= 0 && eos < V, "ngram_score_cands: eos=%d outside [0, V=%d)", eos, V);
  OTR_REQUIRE(alpha == alpha && beta == beta && oov_score == oov_score, "ngram_score_cands: NaN alpha / beta / oov_score");
  OTR_REQUIRE(beam >= 0 && beam <= NA_MAXBEAM && beam <= K, "ngram_score_cands: beam=%d must be in [0, min(%d, K=%d)]", beam, NA_MAXBEAM, K);
  OTR_REQUIRE(beam == 0 || (k_score && k_idx), "ngram_score_cands: null top-beam output");
  if (rows == 0) return 0;
  const NgTable tb{(const uint4*)table, (uint32_t)(capacity - 1), max_probe};
  hipLaunchKernelGGL(ngram_score_cands_kernel, dim3((unsigned)((rows + NA_ROWS - 1) / NA_ROWS)), dim3(256), 0, (hipStream_t)stream, tb, order,
                     V, preds, ldp, t, pos, flags, cand_idx, cand_score, rows, K, alpha, beta, oov_score, eos, cand_out, cand_add, beam, k_score,
                     k_idx);
  return otr_check_launch("ngram_score_cands");
}

// ---------------------------------------------------------------- whole hypotheses
__global__ __launch_bounds__(64) void ngram_score_seqs_kernel(NgTable tb, int order, int V, const int64_t* tokens, const int32_t* out_len, int T,
                                                              float alpha, float beta, float oov_score, int eos, float* out, float* logp) {
  const int lane = threadIdx.x;
  const int64_t h = blockIdx.x;
  const int n = out_len[h];
  if (n < 0 || n > T) {                                 // (uniform) no hypothesis in this slot
    if (lane == 0) {
      out[h] = 0.f;
      if (logp) logp[h] = 0.f;
    }
    return;
  }
  const int64_t* tok = tokens + h * T;
  float acc = 0.f;
  for (int l = lane; l <= n; l += 64) {                 // position l: token l given <s> + tokens[0 : l]; position n is </s>
    const int64_t c = l < n ? tok[l] : (int64_t)eos;
    const int L = min(l + 1, order - 1);
    uint64_t cx = 0;
    bool bad = c < 0 || c > V;
    for (int j = 0; j < L; ++j) {
      const int i = l - 1 - j;
      const int64_t id = i < 0 ? (int64_t)V : tok[i];
      bad |= id < 0 || id > V;
      cx |= (uint64_t)((uint32_t)id & 0xffffu) << (16 * j);
    }
    acc += bad ? oov_score : ng_lookup(tb, cx, L, (int)c, oov_score);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    out[h] = __fadd_rn(__fmul_rn(alpha, acc), __fmul_rn(beta, (float)n));
    if (logp) logp[h] = acc;
  }
}

extern "C" int32_t otr_ngram_score_seqs(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V,
                                        const int64_t* tokens, const int32_t* out_len, int64_t n_hyp, int32_t T, float alpha, float beta,
                                        float oov_score, int32_t eos, float* out, float* logp, void* stream) {
  if (otr_ngram_check_table("ngram_score_seqs", table, capacity, max_probe, order, V) < 0) return -1;
  OTR_REQUIRE(out_len && out && (tokens || T == 0), "ngram_score_seqs: null pointer");
  OTR_REQUIRE(n_hyp >= 0 && n_hyp < (1ll << 31) && T >= 0, "ngram_score_seqs: bad shape n_hyp=%lld T=%d", (long long)n_hyp, T);
  OTR_REQUIRE(eos >= 0 && eos < V, "ngram_score_seqs: eos=%d outside [0, V=%d)", eos, V);
  OTR_REQUIRE(alpha == alpha && beta == beta && oov_score == oov_score, "ngram_score_seqs: NaN alpha / beta / oov_score");
  if (n_hyp == 0) return 0;
  const NgTable tb{(const uint4*)table, (uint32_t)(capacity - 1), max_probe};
  hipLaunchKernelGGL(ngram_score_seqs_kernel, dim3((unsigned)n_hyp), dim3(64), 0, (hipStream_t)stream, tb, order, V, tokens, out_len, T, alpha,
                     beta, oov_score, eos, out, logp);
  return otr_check_launch("ngram_score_seqs");
}
