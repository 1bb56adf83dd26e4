// Backoff n-gram LM on the device: the table lookup behind NGramLM.lookup (opentransformer_amd/ngram.py) and the unit-test surface
// of the table the CTC prefix beam search probes (ctcbeam.hip, otr_ctc_beam_search_lm).  ngram.h holds the layout, the probe and the
// combine; include/otrans_hip.h states the scoring rule.
#include "ngram.h"

// One thread per query.  Every probe the rule can need -- the L+1 n-grams (suffix, tok), the L context suffixes whose backoffs a miss
// adds, and the unigrams of the L-1 older context ids that decide whether the window holds an OOV id -- is issued together, then
// combined: no probe waits for the result of another.
__global__ __launch_bounds__(256) void ngram_lookup_kernel(NgTable t, int order, int V, const int32_t* ctx, const int32_t* ctx_len,
                                                           const int32_t* tok, int64_t n, float oov_score, float* out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int N1 = order - 1;
  const int L = N1 > 0 ? min(max(ctx_len[q], 0), N1) : 0;
  const int c = tok[q];
  bool bad = c < 0 || c > V;
  uint64_t cx = 0;                                     // the context packed newest id first
  for (int j = 0; j < L; ++j) {                        // row q holds its L ids oldest first
    const int id = ctx[q * N1 + j];
    bad |= id < 0 || id > V;
    cx = (cx << 16) | (uint64_t)(uint32_t)(id & 0xffff);
  }
  if (bad) { out[q] = oov_score; return; }
  constexpr int NP = 3 * NG_MAXN - 3;                  // 5 n-grams, 4 context suffixes, 3 older unigrams
  uint64_t klo[NP], khi[NP];
  float lp[NP], bo[NP];
  const uint64_t glo = (cx << 16) | (uint64_t)(uint32_t)c;
  const uint32_t ghi = (uint32_t)(cx >> 48);
#pragma unroll
  for (int k = 0; k < NG_MAXN; ++k) ng_key(glo, ghi, k + 1, klo[k], khi[k]);
#pragma unroll
  for (int k = 1; k < NG_MAXN; ++k) ng_key(cx, 0u, k, klo[NG_MAXN - 1 + k], khi[NG_MAXN - 1 + k]);
#pragma unroll
  for (int j = 1; j < NG_MAXN - 1; ++j) ng_key(cx >> (16 * j), 0u, 1, klo[2 * NG_MAXN - 2 + j], khi[2 * NG_MAXN - 2 + j]);
  uint32_t want = (2u << L) - 1u;                                            // n-grams k = 0 .. L
  want |= ((1u << L) - 1u) << NG_MAXN;                                       // context suffixes k = 1 .. L
  if (L > 1) want |= ((1u << (L - 1)) - 1u) << (2 * NG_MAXN - 1);           // unigrams of context ids 1 .. L-1 (0 = the newest)
  const uint32_t found = ng_find<NP>(t, klo, khi, want, lp, bo);
  uint32_t need = 1u;                                  // the unigrams of tok, of the newest context id and of the older ones
  if (L > 0) need |= 1u << NG_MAXN;
  if (L > 1) need |= ((1u << (L - 1)) - 1u) << (2 * NG_MAXN - 1);
  if ((found & need) != need) {
    out[q] = oov_score;                                // tok, the newest context id or an older one has no unigram
    return;
  }
  float glp[NG_MAXN], cbo[NG_MAXN - 1];
#pragma unroll
  for (int k = 0; k < NG_MAXN; ++k) glp[k] = lp[k];
#pragma unroll
  for (int k = 1; k < NG_MAXN; ++k) cbo[k - 1] = (found >> (NG_MAXN - 1 + k) & 1) ? bo[NG_MAXN - 1 + k] : 0.f;
  out[q] = ng_combine(found, glp, cbo, L);
}

int32_t otr_ngram_check_table(const char* who, const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V) {
  OTR_REQUIRE(table && ((uintptr_t)table & 31) == 0, "%s: the n-gram table must be non-null and 32-byte aligned", who);
  OTR_REQUIRE(capacity >= 2 && capacity <= (1ll << 31) && (capacity & (capacity - 1)) == 0,
              "%s: table capacity %lld must be a power of two in [2, 2^31]", who, (long long)capacity);
  OTR_REQUIRE(max_probe >= 1 && max_probe <= capacity, "%s: max_probe=%d must be in [1, capacity]", who, max_probe);
  OTR_REQUIRE(order >= 1 && order <= NG_MAXN, "%s: n-gram order %d must be in [1, %d]", who, order, NG_MAXN);
  OTR_REQUIRE(V >= 1 && V <= 8192, "%s: V=%d must be in [1, 8192] (ids 0 .. V in 16 bits)", who, V);
  return 0;
}

extern "C" int32_t otr_ngram_lookup(const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V,
                                    const int32_t* ctx, const int32_t* ctx_len, const int32_t* tok, int64_t n, float oov_score,
                                    float* out, void* stream) {
  if (otr_ngram_check_table("ngram_lookup", table, capacity, max_probe, order, V) < 0) return -1;
  OTR_REQUIRE(n >= 0 && n < (1ll << 31) * 256, "ngram_lookup: bad query count %lld", (long long)n);
  if (n == 0) return 0;
  OTR_REQUIRE(tok && out && (order == 1 || (ctx && ctx_len)), "ngram_lookup: null pointer");
  const NgTable t{(const uint4*)table, (uint32_t)(capacity - 1), max_probe};
  hipLaunchKernelGGL(ngram_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, order, V, ctx,
                     ctx_len, tok, n, oov_score, out);
  return otr_check_launch("ngram_lookup");
}
