// Phrase biasing (hotwords) for the attention, joint and two-pass decoders (SpeechToTextRecognizer bias=...).  opentransformer_amd/bias.py
// builds the table; include/otrans_hip.h states the semantics.  f32 and integers only: the same code in both builds.
//
// The table, its probe (bs_child) and the host check of its arguments are bias.h's, shared with the CTC prefix beam search.
//  * bias_score_cands: a row owns 32 lanes.  Lane j <= 16 walks the last j tokens of the prefix from the root; the lanes that arrive
//                      are the suffix chain of state(g), the deepest of them the state itself.  Each candidate lane then asks for
//                      child(n_j, c) from the deepest j down: the first that exists is state(g c).
//  * bias_score_seqs:  one wave per hypothesis, one lane per position; the lane finds the state behind its token, its left neighbour
//                      hands over the state in front of it.  Lane sums, then the wave's butterfly: the same order on every run.
#include "bias.h"

#define NEG_INF (-__builtin_huge_valf())

constexpr int BS_MAXV = 8192;
constexpr int BS_MAXK = 32;       // the pre-beam's K'
constexpr int BS_MAXBEAM = 16;    // the prune's limit
constexpr int BS_ROWS = 8;        // hypothesis rows per workgroup: 32 lanes each

__global__ __launch_bounds__(256) void bias_score_cands_kernel(BsTable tb, int max_len, int V, const int64_t* preds, int64_t ldp, int t_host,
                                                               const int32_t* pos, const uint8_t* flags, const int32_t* cand_idx,
                                                               const float* cand_score, int64_t rows, int K, int eos, float* cand_out,
                                                               float* cand_add, int beam, float* k_score, int64_t* k_idx) {
  const int tid = threadIdx.x, lane = tid & 63, k = tid & 31, base = lane & 32;
  const int64_t row = (int64_t)blockIdx.x * BS_ROWS + (tid >> 5);
  const bool in_row = row < rows;
  const bool fin = in_row && flags && flags[row];
  const bool act = in_row && k < K;                     // this lane holds a candidate
  const bool score = act && !fin;
  int t = pos ? *pos + 1 : t_host;                      // prefix columns: BOS (by position) + t - 1 tokens
  t = min(max(t, 1), (int)min(ldp, (int64_t)0x7fffffff));
  // lane j = k: the node of the last j tokens, if they are one (j = 0: the root).  psi is that node's.
  bool ok = in_row && !fin && k <= min(t - 1, max_len);
  uint32_t node = 0;
  float psi = 0.f;
  for (int i = 0; i < k && ok; ++i) {
    const int64_t id = preds[row * ldp + (t - k + i)];  // columns t - k .. t - 1, all >= 1
    float pm = 0.f;
    bool end = false;
    ok = id >= 0 && id < V && bs_child(tb, node, (uint32_t)id, node, pm, end);
    psi = end ? 0.f : pm;
  }
  const uint32_t chain = (uint32_t)(__ballot(ok) >> base);      // bit j: the last j tokens are a node; 0 on a finished row
  const int deepest = chain ? 31 - __clz(chain) : 0;
  const float psi_g = __shfl(psi, base + deepest);              // psi(state(g))
  const int c = act ? cand_idx[row * K + k] : 0;
  const float cs = act ? cand_score[row * K + k] : NEG_INF;
  const bool probe = score && c >= 0 && c < V;
  bool hit = false;
  float pm_new = 0.f;                                           // psi_minus(state(g c)): the root's where no suffix goes on with c
  for (int q = BS_MAXLEN - 1; q >= 0; --q) {                    // (uniform trip count; a node of depth 16 has no child)
    const uint32_t nq = __shfl(node, base + q);
    if (probe && !hit && (chain >> q & 1u) && q < max_len) {
      uint32_t child;
      float pm = 0.f;
      bool end;
      hit = bs_child(tb, nq, (uint32_t)c, child, pm, end);
      if (hit) pm_new = pm;
    }
  }
  float add = 0.f, out = cs;
  if (score) {
    add = __fsub_rn(pm_new, psi_g);
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

// host: the checks every entry that takes a phrase table shares (bias.h); -1 and the error string on a refusal
int32_t otr_bias_check_table(const char* who, const void* table, int64_t capacity, int32_t max_probe, int32_t max_len) {
  OTR_REQUIRE(table != nullptr, "%s: null table", who);
  OTR_REQUIRE(((uintptr_t)table & 15u) == 0, "%s: table must be 16-byte aligned", who);
  OTR_REQUIRE(capacity >= 2 && capacity <= (1ll << 31) && (capacity & (capacity - 1)) == 0,
              "%s: capacity=%lld must be a power of two in [2, 2^31]", who, (long long)capacity);
  OTR_REQUIRE(max_probe >= 1 && max_probe <= capacity, "%s: max_probe=%d must be in [1, capacity]", who, max_probe);
  OTR_REQUIRE(max_len >= 1 && max_len <= BS_MAXLEN, "%s: max_len=%d must be in [1, %d]", who, max_len, BS_MAXLEN);
  return 0;
}
// the same plus the two arguments only this file's entries take
static int32_t bias_check_table(const char* who, const void* table, int64_t capacity, int32_t max_probe, int32_t n_nodes, int32_t max_len,
                                int32_t V) {
  if (otr_bias_check_table(who, table, capacity, max_probe, max_len) < 0) return -1;
  OTR_REQUIRE(n_nodes >= 2 && (int64_t)n_nodes - 1 <= capacity, "%s: n_nodes=%d must be in [2, capacity + 1]", who, n_nodes);
  OTR_REQUIRE(V >= 1 && V <= BS_MAXV, "%s: V=%d must be in [1, %d]", who, V, BS_MAXV);
  return 0;
}

extern "C" int32_t otr_bias_score_cands(const void* table, int64_t capacity, int32_t max_probe, int32_t n_nodes, int32_t max_len, int32_t V,
                                        const int64_t* preds, int64_t ldp, int32_t t, const int32_t* pos, const uint8_t* flags,
                                        const int32_t* cand_idx, const float* cand_score, int64_t rows, int32_t K, int32_t eos,
                                        float* cand_out, float* cand_add, int32_t beam, float* k_score, int64_t* k_idx, void* stream) {
  if (bias_check_table("bias_score_cands", table, capacity, max_probe, n_nodes, max_len, V) < 0) return -1;
  OTR_REQUIRE(preds && cand_idx && cand_score && cand_out, "bias_score_cands: null pointer");
  OTR_REQUIRE(K >= 1 && K <= BS_MAXK, "bias_score_cands: K=%d must be in [1, %d]", K, BS_MAXK);
  OTR_REQUIRE(rows >= 0 && rows < (1ll << 31), "bias_score_cands: bad rows");
  OTR_REQUIRE(ldp >= 1 && (pos || (t >= 1 && t <= ldp)), "bias_score_cands: t=%d must be in [1, ldp=%lld]", t, (long long)ldp);
  OTR_REQUIRE(eos >= 0 && eos < V, "bias_score_cands: eos=%d outside [0, V=%d)", eos, V);
  OTR_REQUIRE(beam >= 0 && beam <= BS_MAXBEAM && beam <= K, "bias_score_cands: beam=%d must be in [0, min(%d, K=%d)]", beam, BS_MAXBEAM, K);
  OTR_REQUIRE(beam == 0 || (k_score && k_idx), "bias_score_cands: null top-beam output");
  if (rows == 0) return 0;
  const BsTable tb{(const uint4*)table, (uint32_t)(capacity - 1), max_probe};
  hipLaunchKernelGGL(bias_score_cands_kernel, dim3((unsigned)((rows + BS_ROWS - 1) / BS_ROWS)), dim3(256), 0, (hipStream_t)stream, tb, max_len,
                     V, preds, ldp, t, pos, flags, cand_idx, cand_score, rows, K, eos, cand_out, cand_add, beam, k_score, k_idx);
  return otr_check_launch("bias_score_cands");
}

// ---------------------------------------------------------------- whole hypotheses
// state(tok[0 : n)): the longest suffix that is a node, tried from the deepest down; pm / ps = its psi_minus / psi (the root: 0, 0)
__device__ __forceinline__ void bs_state(const BsTable& tb, const int64_t* tok, int n, int max_len, int V, float& pm, float& ps) {
  pm = ps = 0.f;
  for (int j = min(n, max_len); j >= 1; --j) {
    uint32_t node = 0;
    float m = 0.f;
    bool end = false, ok = true;
    for (int i = 0; i < j && ok; ++i) {
      const int64_t id = tok[n - j + i];
      ok = id >= 0 && id < V && bs_child(tb, node, (uint32_t)id, node, m, end);
    }
    if (ok) {
      pm = m;
      ps = end ? 0.f : m;
      return;
    }
  }
}

__global__ __launch_bounds__(64) void bias_score_seqs_kernel(BsTable tb, int max_len, int V, const int64_t* tokens, const int32_t* out_len,
                                                             int T, float* out) {
  const int lane = threadIdx.x;
  const int64_t h = blockIdx.x;
  const int n = out_len[h];
  if (n < 0 || n > T) {                                 // (uniform) no hypothesis in this slot
    if (lane == 0) out[h] = 0.f;
    return;
  }
  const int64_t* tok = tokens + h * T;
  float acc = 0.f, carry = 0.f;                         // carry: psi of the state in front of the chunk (the root's at the start)
  for (int l0 = 0; l0 <= n; l0 += 64) {                 // (uniform) position l: token l behind tokens[0 : l]; position n is EOS
    const int l = l0 + lane;
    float pm = 0.f, ps = 0.f;                           // of state(tokens[0 : l + 1]); behind EOS it is the root
    if (l < n) bs_state(tb, tok, l + 1, max_len, V, pm, ps);
    float prev = __shfl_up(ps, 1);
    if (lane == 0) prev = carry;
    if (l <= n) acc = __fadd_rn(acc, __fsub_rn(pm, prev));
    carry = __shfl(ps, 63);
  }
  acc = wave_sum(acc);
  if (lane == 0) out[h] = acc;
}

extern "C" int32_t otr_bias_score_seqs(const void* table, int64_t capacity, int32_t max_probe, int32_t n_nodes, int32_t max_len, int32_t V,
                                       const int64_t* tokens, const int32_t* out_len, int64_t n_hyp, int32_t T, int32_t eos, float* out,
                                       void* stream) {
  if (bias_check_table("bias_score_seqs", table, capacity, max_probe, n_nodes, max_len, V) < 0) return -1;
  OTR_REQUIRE(out_len && out && (tokens || T == 0), "bias_score_seqs: null pointer");
  OTR_REQUIRE(n_hyp >= 0 && n_hyp < (1ll << 31) && T >= 0, "bias_score_seqs: bad shape n_hyp=%lld T=%d", (long long)n_hyp, T);
  OTR_REQUIRE(eos >= 0 && eos < V, "bias_score_seqs: eos=%d outside [0, V=%d)", eos, V);
  if (n_hyp == 0) return 0;
  const BsTable tb{(const uint4*)table, (uint32_t)(capacity - 1), max_probe};
  hipLaunchKernelGGL(bias_score_seqs_kernel, dim3((unsigned)n_hyp), dim3(64), 0, (hipStream_t)stream, tb, max_len, V, tokens, out_len, T, out);
  return otr_check_launch("bias_score_seqs");
}
