// n-gram LM estimation on the device (NGramLM.train, opentransformer_amd/ngram.py): interpolated modified Kneser-Ney from unit-id
// sentences.  include/otrans_hip.h states the count-entry layout, the estimator and the error bits; ngram.h holds the hash the count
// table shares with the scoring table.  Integers, f32 and f64 only: the same code in both library builds.
//
// Nothing here takes a lock or waits for another thread.  An insertion is one 64-bit compare-and-swap on the key word (0 = empty, a
// key never changes once it is set) followed by integer atomic adds; every probe loop is bounded by the capacity and a full table
// raises an error bit.  Every statistic is an integer sum and every float a pure function of the integers, so the results do not
// depend on the order of threads, entries or sentences.
#include "ngram.h"

constexpr int NT_MAXN = 4;   // highest order: four 16-bit ids in the one key word
enum { NT_ERR_FULL = 1, NT_ERR_ID = 2, NT_ERR_LEN = 4, NT_ERR_MISSING = 8 };

struct NtEntry {             // 32 bytes
  unsigned long long key;    // ids newest first, 16 bits each; 0 = empty
  uint32_t raw, cont;        // c(g); distinct (m+1)-grams that end in g
  uint32_t sum, n1, n2, n3p; // statistics of g as a context
};
struct NtDisc {
  double cur[3], next[3];    // D_m[1..3] of the launch's order m, and of order m+1 (the backoffs)
};

__device__ __forceinline__ int nt_order(uint64_t key) { return key >> 48 ? 4 : key >> 32 ? 3 : key >> 16 ? 2 : 1; }
__device__ __forceinline__ uint64_t nt_newest(uint64_t key, int m) { return m >= 4 ? key : key & ((1ull << (16 * m)) - 1ull); }
__device__ __forceinline__ uint32_t nt_home(uint64_t key, int m, uint32_t mask) {
  return (uint32_t)ng_hash(key, (uint64_t)m << 16) & mask;
}

// the entry of `key` (order m), claimed if no thread has yet; -1: the table is full.  created: this call's compare-and-swap made it
__device__ __forceinline__ int64_t nt_insert(NtEntry* t, uint32_t mask, uint64_t key, int m, bool& created) {
  uint32_t pos = nt_home(key, m, mask);
  created = false;
  for (uint64_t p = 0; p <= mask; ++p) {
    unsigned long long* kp = &t[pos].key;
    unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {          // a stale 0 is settled by the compare-and-swap; a non-zero key is final
      cur = atomicCAS(kp, 0ull, (unsigned long long)key);
      if (cur == 0) {
        created = true;
        return pos;
      }
    }
    if (cur == key) return pos;
    pos = (pos + 1) & mask;
  }
  return -1;
}
// read only (the passes after the count): -1 if the key is not stored
__device__ __forceinline__ int64_t nt_find(const NtEntry* t, uint32_t mask, uint64_t key, int m) {
  uint32_t pos = nt_home(key, m, mask);
  for (uint64_t p = 0; p <= mask; ++p) {
    const unsigned long long cur = t[pos].key;
    if (cur == key) return pos;
    if (cur == 0) return -1;
    pos = (pos + 1) & mask;
  }
  return -1;
}
// a(g): the raw count at the highest order and for a gram that starts with <s>, the continuation count otherwise
__device__ __forceinline__ uint32_t nt_adjusted(const NtEntry& e, int m, int N, int V) {
  return (m == N || (int)((e.key >> (16 * (m - 1))) & 0xffff) == V) ? e.raw : e.cont;
}

// One thread per (sentence, end position i of x = <s> w_1 .. w_n </s>): the grams x[i-m+1 .. i], m = 1 .. min(N, i+1), shortest first.
__global__ __launch_bounds__(256) void ngram_count_kernel(const int64_t* tokens, int64_t ld, const int32_t* lengths, int64_t n_sent,
                                                          int max_len, int N, int V, int eos, NtEntry* t, uint32_t mask, int32_t* err) {
  const int P = max_len + 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_sent * P) return;
  const int64_t b = idx / P;
  const int i = (int)(idx - b * P);
  const int len = lengths[b];
  if (len < 0 || len > max_len) {
    if (i == 0) atomicOr(err, NT_ERR_LEN);
    return;
  }
  if (i > len + 1) return;
  const int M = min(N, i + 1);
  uint64_t key = 0;
  bool bad = false;
  for (int k = 0; k < M; ++k) {                         // x[i - k] into field k; columns >= len are never read
    const int j = i - k;
    int id = j == 0 ? V : eos;
    if (j >= 1 && j <= len) {
      const int64_t tok = tokens[b * ld + (j - 1)];
      bad |= tok < 1 || tok >= V || tok == eos;
      id = (int)(tok & 0xffff);
    }
    key |= (uint64_t)(uint32_t)id << (16 * k);
  }
  if (bad) {
    atomicOr(err, NT_ERR_ID);
    return;
  }
  int64_t prev = -1;
  for (int m = 1; m <= M; ++m) {
    bool created;
    const int64_t s = nt_insert(t, mask, nt_newest(key, m), m, created);
    if (s < 0) {
      atomicOr(err, NT_ERR_FULL);
      return;
    }
    atomicAdd(&t[s].raw, 1u);
    if (created && m > 1) atomicAdd(&t[prev].cont, 1u);   // a new (m)-gram: one more distinct left extension of its suffix
    prev = s;
  }
}

// One thread per entry: a(g) into the statistics of its context (the key without its newest id) and into the count-of-counts.  The
// empty context and the count-of-counts are single words for the whole grid: summed in LDS per workgroup, one atomic per word after.
__global__ __launch_bounds__(256) void ngram_stats_kernel(NtEntry* t, uint32_t mask, int64_t cap, int N, int V,
                                                          unsigned long long* glob, int32_t* err) {
  __shared__ unsigned long long acc[20];
  if (threadIdx.x < 20) acc[threadIdx.x] = 0;
  __syncthreads();
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot < cap) {
    const NtEntry e = t[slot];
    if (e.key != 0 && e.key != (uint64_t)V) {          // the unigram <s> takes part in nothing
      const int m = nt_order(e.key);
      const uint32_t a = m <= N ? nt_adjusted(e, m, N, V) : 0u;
      if (a == 0) {
        atomicOr(err, NT_ERR_MISSING);
      } else {
        const int k = a >= 3 ? 2 : (int)a - 1;
        if (a <= 4) atomicAdd(&acc[4 + 4 * (m - 1) + (a - 1)], 1ull);
        if (m == 1) {
          atomicAdd(&acc[0], (unsigned long long)a);
          atomicAdd(&acc[1 + k], 1ull);
        } else {
          const int64_t c = nt_find(t, mask, e.key >> 16, m - 1);
          if (c < 0) {
            atomicOr(err, NT_ERR_MISSING);
          } else {
            atomicAdd(&t[c].sum, a);
            atomicAdd(&t[c].n1 + k, 1u);                 // n1, n2, n3p are consecutive words
          }
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 20 && acc[threadIdx.x]) atomicAdd(&glob[threadIdx.x], acc[threadIdx.x]);
}

// One thread per entry, the entries of order m only: p_m from the integers and the stored p_{m-1} of the suffix, and the backoff.
__global__ __launch_bounds__(256) void ngram_estimate_kernel(const NtEntry* t, uint32_t mask, int64_t cap, int m, int N, int V,
                                                             double p0, NtDisc d, const unsigned long long* glob, double* prob,
                                                             float* logp, float* backoff, int32_t* err) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= cap) return;
  const NtEntry e = t[slot];
  if (e.key == 0 || nt_order(e.key) != m) return;
  float bo = 0.f;
  if (m < N && e.sum > 0)
    bo = (float)log((d.next[0] * (double)e.n1 + d.next[1] * (double)e.n2 + d.next[2] * (double)e.n3p) / (double)e.sum);
  backoff[slot] = bo;
  if (e.key == (uint64_t)V) {                            // the unigram <s>: ARPA's -99
    prob[slot] = 0.0;
    logp[slot] = (float)(-99.0 * 2.302585092994046);
    return;
  }
  const uint32_t a = nt_adjusted(e, m, N, V);
  double sum, n1, n2, n3p, lower = p0;
  if (m == 1) {
    sum = (double)glob[0], n1 = (double)glob[1], n2 = (double)glob[2], n3p = (double)glob[3];
  } else {
    const int64_t c = nt_find(t, mask, e.key >> 16, m - 1), s = nt_find(t, mask, nt_newest(e.key, m - 1), m - 1);
    if (c < 0 || s < 0 || t[c].sum == 0 || a == 0) {
      atomicOr(err, NT_ERR_MISSING);
      return;
    }
    sum = (double)t[c].sum, n1 = (double)t[c].n1, n2 = (double)t[c].n2, n3p = (double)t[c].n3p;
    lower = prob[s];
  }
  const double gamma = (d.cur[0] * n1 + d.cur[1] * n2 + d.cur[2] * n3p) / sum;
  const double p = ((double)a - d.cur[a >= 3 ? 2 : (int)a - 1]) / sum + gamma * lower;
  prob[slot] = p;
  logp[slot] = (float)log(p);
}

static int32_t nt_check(const char* who, const void* table, int64_t capacity, int32_t order, int32_t V, const void* err) {
  OTR_REQUIRE(table && ((uintptr_t)table & 7) == 0, "%s: the count table must be non-null and 8-byte aligned", who);
  OTR_REQUIRE(capacity >= 2 && capacity <= (1ll << 31) && (capacity & (capacity - 1)) == 0,
              "%s: table capacity %lld must be a power of two in [2, 2^31]", who, (long long)capacity);
  OTR_REQUIRE(order >= 1 && order <= NT_MAXN, "%s: n-gram order %d must be in [1, %d]", who, order, NT_MAXN);
  OTR_REQUIRE(V >= 1 && V <= 8192, "%s: V=%d must be in [1, 8192] (ids 0 .. V in 16 bits)", who, V);
  OTR_REQUIRE(err != nullptr, "%s: null error word", who);
  return 0;
}

extern "C" int32_t otr_ngram_count(const int64_t* tokens, int64_t ld, const int32_t* lengths, int64_t n_sent, int32_t max_len,
                                   int32_t order, int32_t V, int32_t eos, void* table, int64_t capacity, int32_t* err, void* stream) {
  if (nt_check("ngram_count", table, capacity, order, V, err) < 0) return -1;
  OTR_REQUIRE(eos >= 1 && eos < V, "ngram_count: the </s> unit %d must be in [1, V = %d)", eos, V);
  OTR_REQUIRE(n_sent >= 0 && max_len >= 0 && ld >= max_len, "ngram_count: bad sizes n_sent=%lld max_len=%d ld=%lld", (long long)n_sent,
              max_len, (long long)ld);
  OTR_REQUIRE(n_sent <= ((1ll << 31) - 1) * 256 / ((int64_t)max_len + 2), "ngram_count: %lld sentences of up to %d ids exceed one grid",
              (long long)n_sent, max_len);
  if (n_sent == 0) return 0;
  OTR_REQUIRE(lengths && (tokens || max_len == 0), "ngram_count: null pointer");
  const int64_t n = n_sent * ((int64_t)max_len + 2);
  hipLaunchKernelGGL(ngram_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tokens, ld, lengths,
                     n_sent, max_len, order, V, eos, (NtEntry*)table, (uint32_t)(capacity - 1), err);
  return otr_check_launch("ngram_count");
}

extern "C" int32_t otr_ngram_stats(void* table, int64_t capacity, int32_t order, int32_t V, uint64_t* glob, int32_t* err, void* stream) {
  if (nt_check("ngram_stats", table, capacity, order, V, err) < 0) return -1;
  OTR_REQUIRE(glob && ((uintptr_t)glob & 7) == 0, "ngram_stats: glob must be non-null and 8-byte aligned");
  hipLaunchKernelGGL(ngram_stats_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (NtEntry*)table,
                     (uint32_t)(capacity - 1), capacity, order, V, (unsigned long long*)glob, err);
  return otr_check_launch("ngram_stats");
}

extern "C" int32_t otr_ngram_estimate(const void* table, int64_t capacity, int32_t order, int32_t V, int32_t n_units,
                                      const double* discounts, const uint64_t* glob, double* prob, float* logp, float* backoff,
                                      int32_t* err, void* stream) {
  if (nt_check("ngram_estimate", table, capacity, order, V, err) < 0) return -1;
  OTR_REQUIRE(n_units >= 1 && n_units <= (V > 1 ? V - 1 : 1), "ngram_estimate: %d predictable units, 1 .. V-1 expected at V = %d", n_units, V);
  OTR_REQUIRE(discounts && glob && prob && logp && backoff, "ngram_estimate: null pointer");
  OTR_REQUIRE(((uintptr_t)glob & 7) == 0 && ((uintptr_t)prob & 7) == 0, "ngram_estimate: glob and prob must be 8-byte aligned");
  for (int i = 0; i < order * 3; ++i)
    OTR_REQUIRE(discounts[i] >= 0.0 && discounts[i] <= (double)(i % 3 + 1), "ngram_estimate: discount D_%d[%d] = %g must be in [0, %d]",
                i / 3 + 1, i % 3 + 1, discounts[i], i % 3 + 1);
  for (int m = 1; m <= order; ++m) {
    NtDisc d;
    for (int k = 0; k < 3; ++k) {
      d.cur[k] = discounts[(m - 1) * 3 + k];
      d.next[k] = m < order ? discounts[m * 3 + k] : 0.0;
    }
    hipLaunchKernelGGL(ngram_estimate_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const NtEntry*)table, (uint32_t)(capacity - 1), capacity, m, order, V, 1.0 / (double)n_units, d,
                       (const unsigned long long*)glob, prob, logp, backoff, err);
    if (int32_t r = otr_check_launch("ngram_estimate")) return r;
  }
  return 0;
}
