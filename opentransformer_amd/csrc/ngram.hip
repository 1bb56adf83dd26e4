// Backoff n-gram LM on the device: the table lookup behind NGramLM.lookup (opentransformer_amd/ngram.py) and the unit-test surface
// of the table the CTC prefix beam search probes (ctcbeam.hip, otr_ctc_beam_search_lm).  ngram.h holds the layout, the probe and the
// combine; include/otrans_hip.h states the scoring rule.
#include "ngram.h"

// One thread per query (ngram.h ng_lookup: every probe the rule can need is issued together, then combined).
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
  out[q] = ng_lookup(t, cx, L, c, oov_score);
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
