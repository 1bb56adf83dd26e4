// Backoff n-gram table on the device (opentransformer_amd/ngram.py builds it; include/otrans_hip.h states the layout and the
// scoring rule).  Shared by the lookup kernel (ngram.hip) and the LM path of the CTC prefix beam search (ctcbeam.hip).
//
// An n-gram w_0 .. w_{m-1} (m <= 5, ids <= 8192 in 16 bits each) is packed newest id first: id w_{m-1-j} at bits [16j, 16j+16) of
// an 80-bit value; key = {lo: bits 0-63, hi: bits 64-79 | m << 16}.  hi != 0 for every stored key, hi == 0 marks an empty entry.
// With a context held the same way (newest id at the bottom) every key a query needs is a shift and a mask of one register pair.
// Entry (32 bytes, 32-byte aligned): u64 lo, u64 hi, f32 log-prob, f32 backoff, 8 bytes of padding.  Open addressing, linear
// probing, capacity a power of two, nothing is ever deleted: a probe chain ends at the key, at an empty entry, or after max_probe
// entries (the longest chain of the build).
#pragma once
#include "common.h"

constexpr int NG_MAXN = 5;   // highest order

// host: the checks every entry that takes a table shares (ngram.hip); -1 and the error string on a refusal
int32_t otr_ngram_check_table(const char* who, const void* table, int64_t capacity, int32_t max_probe, int32_t order, int32_t V);

struct NgTable {
  const uint4* e;       // capacity entries of two uint4 each
  uint32_t mask;        // capacity - 1
  int max_probe;
};

__device__ __forceinline__ uint64_t ng_hash(uint64_t lo, uint64_t hi) {   // ngram.py _hash: the same arithmetic in numpy
  uint64_t z = lo ^ (hi * 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// key of the m newest ids (1 <= m <= 5) of the packed value {lo, hi16}
__device__ __forceinline__ void ng_key(uint64_t lo, uint32_t hi16, int m, uint64_t& klo, uint64_t& khi) {
  klo = m >= 4 ? lo : lo & ((1ull << (16 * m)) - 1ull);
  khi = (uint64_t)((m == 5 ? hi16 : 0u) | ((uint32_t)m << 16));
}

// NP independent lookups.  The first probe of every wanted key is issued before any of them is looked at; a key whose home entry
// holds another key walks on, all unresolved keys one entry per round.  Returns the mask of keys found; lp / bo are written for those.
template <int NP>
__device__ __forceinline__ uint32_t ng_find(const NgTable& t, const uint64_t (&klo)[NP], const uint64_t (&khi)[NP], uint32_t want,
                                            float (&lp)[NP], float (&bo)[NP]) {
  uint32_t pos[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) pos[j] = (uint32_t)ng_hash(klo[j], khi[j]) & t.mask;
  uint32_t found = 0, open = want;
  for (int p = 0; p < t.max_probe && open; ++p) {
    uint4 k[NP], v[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (open >> j & 1) {
        k[j] = ld_global_b128(t.e + 2 * (size_t)pos[j]);
        v[j] = ld_global_b128(t.e + 2 * (size_t)pos[j] + 1);
      }
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (open >> j & 1) {
        const uint64_t elo = (uint64_t)k[j].x | ((uint64_t)k[j].y << 32), ehi = (uint64_t)k[j].z | ((uint64_t)k[j].w << 32);
        if (elo == klo[j] && ehi == khi[j]) {
          found |= 1u << j;
          open &= ~(1u << j);
          lp[j] = __uint_as_float(v[j].x);
          bo[j] = __uint_as_float(v[j].y);
        } else if (ehi == 0) {
          open &= ~(1u << j);
        } else {
          pos[j] = (pos[j] + 1) & t.mask;
        }
      }
  }
  return found;
}

// The n-grams (newest k ids of the context, c), k = 0 .. L: bit k of the result says that one is stored, lp[k] / bo[k] are its
// log-prob and its backoff.  ctx: the context's ids packed newest first (<= 4 ids), L <= NG_MAXN - 1 its length.
__device__ __forceinline__ uint32_t ng_probe_grams(const NgTable& t, uint64_t ctx, int L, int c, float (&lp)[NG_MAXN],
                                                   float (&bo)[NG_MAXN]) {
  const uint64_t lo = (ctx << 16) | (uint64_t)(uint32_t)c;
  const uint32_t hi16 = (uint32_t)(ctx >> 48);
  uint64_t klo[NG_MAXN], khi[NG_MAXN];
#pragma unroll
  for (int k = 0; k < NG_MAXN; ++k) ng_key(lo, hi16, k + 1, klo[k], khi[k]);
  return ng_find<NG_MAXN>(t, klo, khi, (2u << L) - 1u, lp, bo);
}

// ln P(c | context) from the probes: the longest stored (suffix, c) plus the backoffs of the longer suffixes, added longest first.
// found: ng_probe_grams' mask (bit 0, the unigram, must be set); ctx_bo[k - 1] = backoff of the newest k ids, 0 where not stored.
__device__ __forceinline__ float ng_combine(uint32_t found, const float (&lp)[NG_MAXN], const float* ctx_bo, int L) {
  float acc = 0.f;
  for (int k = L; k > 0; --k) {
    if (found >> k & 1) return acc + lp[k];
    acc += ctx_bo[k - 1];
  }
  return acc + lp[0];
}

// ln P(c | context) for one query that shares nothing with its neighbours (the lookup kernel, the sentence scorer).  Every probe the
// rule can need -- the L+1 n-grams (suffix, c), the L context suffixes whose backoffs a miss adds, and the unigrams of the L-1 older
// context ids that decide whether the window holds an OOV id -- is issued together, then combined: no probe waits for the result
// of another.  cx: the context packed newest id first, every id in [0, V]; 0 <= L <= NG_MAXN - 1; c in [0, V].
__device__ __forceinline__ float ng_lookup(const NgTable& t, uint64_t cx, int L, int c, float oov_score) {
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
  uint32_t need = 1u;                                  // the unigrams of c, of the newest context id and of the older ones
  if (L > 0) need |= 1u << NG_MAXN;
  if (L > 1) need |= ((1u << (L - 1)) - 1u) << (2 * NG_MAXN - 1);
  if ((found & need) != need) return oov_score;        // c, the newest context id or an older one has no unigram
  float glp[NG_MAXN], cbo[NG_MAXN - 1];
#pragma unroll
  for (int k = 0; k < NG_MAXN; ++k) glp[k] = lp[k];
#pragma unroll
  for (int k = 1; k < NG_MAXN; ++k) cbo[k - 1] = (found >> (NG_MAXN - 1 + k) & 1) ? bo[NG_MAXN - 1 + k] : 0.f;
  return ng_combine(found, glp, cbo, L);
}
