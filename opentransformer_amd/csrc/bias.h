// Phrase-biasing table on the device (opentransformer_amd/bias.py builds it; include/otrans_hip.h states the layout and the rule).
// Shared by the candidate / sequence kernels (bias.hip) and the phrase path of the CTC prefix beam search (ctcbeam.hip).
//
// Table: the edges (node, token) -> child of the phrases' trie, open addressing, linear probing, capacity a power of two, nothing is
// ever deleted.  Entry (16 bytes): u32 node + 1 (0 = empty), u32 token | end(child) << 31, u32 child, f32 psi_minus(child).  What a
// step needs of a node -- psi_minus, and psi = end ? 0 : psi_minus -- travels with the edge that reaches it, so a node number is only
// ever a key, never an index: no probe can leave the table whatever it holds.  No failure links: the device walks goto edges only.
#pragma once
#include "common.h"

constexpr int BS_MAXLEN = 16;     // BIAS_MAX_LEN: ids per phrase, the depth of the trie

// host: the table checks every entry that takes a phrase table shares (bias.hip); -1 and the error string on a refusal
int32_t otr_bias_check_table(const char* who, const void* table, int64_t capacity, int32_t max_probe, int32_t max_len);

struct BsTable {
  const uint4* e;
  uint32_t mask;        // capacity - 1
  int max_probe;
};

__device__ __forceinline__ uint32_t bs_hash(uint32_t node, uint32_t tok) {   // bias.py _hash: the same arithmetic in numpy
  uint64_t z = (((uint64_t)node << 16) | (uint64_t)tok) * 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)(z ^ (z >> 31));
}

// the edge (node, tok): true where it is stored, with the child, psi_minus(child) and end(child).  0 <= tok < 8192.
__device__ __forceinline__ bool bs_child(const BsTable& t, uint32_t node, uint32_t tok, uint32_t& child, float& pm, bool& end) {
  uint32_t pos = bs_hash(node, tok) & t.mask;
  for (int p = 0; p < t.max_probe; ++p) {
    const uint4 e = ld_global_b128(t.e + pos);
    if (e.x == node + 1u && (e.y & 0x7fffffffu) == tok) {
      child = e.z;
      pm = __uint_as_float(e.w);
      end = (e.y >> 31) != 0u;
      return true;
    }
    if (e.x == 0u) return false;
    pos = (pos + 1u) & t.mask;
  }
  return false;
}
