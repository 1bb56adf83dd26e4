// CTC prefix beam search on the device: the decoder behind CTCRecognizer(mode='beam') (recognize/ctc.py:60-67, which hands it to
// the un-vendored ctcdecode_edited).  Two launches per batch, f32 in both builds; include/otrans_hip.h states the semantics.
//  * ctc_topk:        one wave per frame (b, t < lengths[b]): the K best (log-prob, token) of the row, descending, ties -> lower
//                     token.  The row sits in registers as order-preserving u32 keys; the K-th largest key is found by a 32-step
//                     bitwise search over wave-wide counts, then the <= K winners are compacted and ranked in LDS.
//  * ctc_beam_search: one workgroup per utterance runs every frame.  Beam state (pb, pnb, last token, length, prefix hash, parent
//                     hash, trie node) lives in LDS; the back-pointer trie {parent node, token} lives in the caller's workspace and
//                     is walked once after the last frame to write the hypotheses.  The kernel is a template: <false> is the plain
//                     search, <true> (otr_ctc_beam_search_lm) adds the n-gram LM addend of include/otrans_hip.h to every
//                     extension.  There a slot also carries its LM context (ids, the backoffs of its suffixes, an OOV mask),
//                     the addend of its last token and its summed LM score; the table (ngram.h) is probed once per
//                     (slot, candidate) in step 1 and once per new slot in step 3.  The second flag, <LM, true>
//                     (otr_ctc_beam_search_bias), adds the phrase-biasing addend of bias.h behind the n-gram's: a slot then also
//                     carries the suffix chain of its phrase state (16 nodes + a mask), psi of that state and its summed phrase
//                     addends; the phrase table is probed in the same two places, and after the last frame the open matches are
//                     refunded and the beam is ranked again.
#include "bias.h"
#include "ngram.h"

#define NEG_INF (-__builtin_huge_valf())

constexpr int CB_MAXW = 32;                            // beam width
constexpr int CB_MAXK = 128;                           // cutoff_top_n: ctcdecode's 40, or every token of a vocabulary <= 128
constexpr int CB_MAXV = 8192;                          // vocabulary of the top-K pass (128 keys per lane)
constexpr int CB_NT = 256;                             // threads of the search workgroup
constexpr int CB_MAXC = CB_MAXW + CB_MAXW * CB_MAXW;   // candidates of a frame after the per-slot cut: W stays + W extensions per slot
constexpr uint64_t CB_H0 = 0x6a09e667f3bcc908ull;      // hash of the empty prefix

// ---------------------------------------------------------------- top-K of a frame
// Order-preserving key of a float: a > b <=> key(a) > key(b).  -0 is folded onto +0 first.  The value 0 is never a key of a
// real float, so it pads the lanes past V.
__device__ __forceinline__ uint32_t cb_key(float x) {
  const uint32_t u = __float_as_uint(x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cb_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NV>
__global__ __launch_bounds__(64) void ctc_topk_kernel(const float* lp, int64_t ld, const int32_t* lengths, int T, int V, int K,
                                                      float* out_lp, int32_t* out_tok) {
  __shared__ uint32_t s_key[CB_MAXK];
  __shared__ int s_tok[CB_MAXK];
  const int64_t row = blockIdx.x;
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  if (t >= lengths[b]) return;                         // frames past the utterance are not read (the search never reads them)
  const int lane = threadIdx.x;
  const float* x = lp + row * ld;
  uint32_t key[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    key[j] = v < V ? cb_key(x[v]) : 0u;
  }
  // tau = the largest key with at least K keys >= it, i.e. the K-th largest key
  uint32_t tau = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = tau | (1u << bit);
    int c = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) c += key[j] >= cand;
    if (wave_isum(c) >= K) tau = cand;
  }
  int gt = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) gt += key[j] > tau;
  const int need_eq = K - wave_isum(gt);               // >= 1: how many keys equal to tau are taken, lowest tokens first
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  int base = 0, eq_seen = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {                       // token v = lane + 64 j: ascending over (j, lane)
    const bool eq = key[j] == tau;
    const uint64_t eqm = __ballot(eq);
    const bool sel = key[j] > tau || (eq && eq_seen + __popcll(eqm & lt_mask) < need_eq);
    const uint64_t selm = __ballot(sel);
    if (sel) {
      const int p = base + __popcll(selm & lt_mask);
      s_key[p] = key[j];
      s_tok[p] = lane + 64 * j;
    }
    base += __popcll(selm);
    eq_seen += __popcll(eqm);
  }
  __syncthreads();                                     // one wave per workgroup: orders the LDS writes before the reads
  for (int e = lane; e < K; e += 64) {
    const uint32_t k = s_key[e];
    const int tok = s_tok[e];
    int r = 0;
    for (int q = 0; q < K; ++q) {
      const uint32_t k2 = s_key[q];
      r += k2 > k || (k2 == k && s_tok[q] < tok);
    }
    out_lp[row * K + r] = cb_unkey(k);
    out_tok[row * K + r] = tok;
  }
}

// ---------------------------------------------------------------- the search
__device__ __forceinline__ float cb_lae(float a, float b) {   // log(exp a + exp b)
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + log1pf(expf(fminf(a, b) - m));
}
__device__ __forceinline__ uint64_t cb_hash(uint64_t h, int c) {   // prefix hash of (prefix with hash h) + token c: splitmix64 finaliser
  uint64_t z = h ^ ((uint64_t)(c + 1) * 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// candidate order: higher score first, then the lower key = (parent slot << 16) | (token + 1), a stay having token -1
__device__ __forceinline__ bool cb_better(float s, int key, float s2, int key2) { return s > s2 || (s == s2 && key < key2); }
struct CbPair { float s; int k; };   // (score, token) of an extension / (score, key) of a candidate: one 8-byte LDS read per compare

struct CbLm {          // the LM path's arguments (unused by the plain instantiation)
  NgTable t;
  int order, V;        // V = the id of <s>
  float alpha, beta, oov_score;
  float* lm_scores;
};
// alpha * ln P(c | context) + beta from the probes of (context suffix, c): `bad` = the context window holds an OOV id
__device__ __forceinline__ float cb_addend(const CbLm& lm, uint32_t found, const float (&lp)[NG_MAXN], const float* ctx_bo, int L, bool bad) {
  const float p = (bad || !(found & 1u)) ? lm.oov_score : ng_combine(found, lp, ctx_bo, L);
  return lm.alpha * p + lm.beta;
}

struct CbBias {        // the phrase path's arguments (unused where BIAS is false)
  BsTable t;
  int max_len;
  float* bias_scores;
};
// state(s c) from the suffix chain of state(s): child(n_j, c) from the deepest chain entry down to the root, the first that exists.
// mask: bit j = the last j tokens of s are a node (bit 0, the root, always); nodes[j - 1] = that node.  Returns psi_minus(state(s c)),
// the root's 0 where no suffix goes on with c.  A node of depth max_len has no child and is not asked.
__device__ __forceinline__ float cb_bias_next(const CbBias& bz, uint32_t mask, const uint32_t* nodes, int c) {
  uint32_t m = mask & ((1u << bz.max_len) - 1u);       // max_len <= 16
  while (m) {
    const int j = 31 - __clz(m);
    m &= ~(1u << j);
    uint32_t child;
    float pm = 0.f;
    bool end;
    if (bs_child(bz.t, j ? nodes[j - 1] : 0u, (uint32_t)c, child, pm, end)) return pm;
  }
  return 0.f;
}

template <bool LM, bool BIAS>
__global__ __launch_bounds__(CB_NT) void ctc_beam_search_kernel(const float* top_lp, const int32_t* top_tok, const int32_t* lengths,
                                                               int T, int K, int blank, int W, int2* trie, int64_t* tokens,
                                                               int32_t* out_len, float* scores, CbLm lm, CbBias bz) {
  constexpr int LW = LM ? CB_MAXW : 1;
  constexpr int BW = BIAS ? CB_MAXW : 1;
  constexpr int AW = (LM || BIAS) ? CB_MAXW : 1;
  __shared__ uint32_t s_bn[2][BW][BS_MAXLEN];          // phrase state: the node of the last j tokens at [j - 1], where s_bm has bit j
  __shared__ uint32_t s_bm[2][BW];                     // bit j (0 .. 16): the last j tokens are a node; bit 0 (the root) always
  __shared__ float s_bpsi[2][BW], s_bs[2][BW];         // psi(state(s)); the summed phrase addends
  __shared__ float s_fin[BW];                          // after the last frame: the refunded scores
  __shared__ int s_perm[BW];                           //   and output row -> slot
  __shared__ uint64_t s_cx[2][LW];                     // LM context: <s> + prefix cut to its newest order-1 ids, newest id lowest
  __shared__ float s_bo[2][LW][NG_MAXN - 1];           // backoff of the newest k ids of the context at [k - 1], 0 where not stored
  __shared__ int s_cl[2][LW];                          // context length | OOV mask << 8 (bit j: the j-th newest id has no unigram)
  __shared__ float s_add[2][AW], s_lm[2][LW];          // addend of the slot's last token, LM + phrase (the 1b merge adds it); summed LM addends
  __shared__ float f_lp[CB_MAXK];
  __shared__ int f_tok[CB_MAXK];
  __shared__ float s_pb[2][CB_MAXW], s_pnb[2][CB_MAXW];
  __shared__ int s_last[2][CB_MAXW], s_len[2][CB_MAXW], s_node[2][CB_MAXW];
  __shared__ uint64_t s_h[2][CB_MAXW], s_ph[2][CB_MAXW];
  __shared__ float st_pb[CB_MAXW], st_pnb[CB_MAXW];    // the stays' new pb / pnb
  __shared__ CbPair x_s[CB_MAXW * CB_MAXK];            // extension (slot i, candidate k): score (-inf = none or merged into a stay), token
  __shared__ CbPair c_s[CB_MAXC];                      // the frame's candidates: score, key
  __shared__ int s_n[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lengths[b], 0), T);
  int2* tr = trie + (int64_t)b * T * W;
  if (tid == 0) {
    s_pb[0][0] = 0.f; s_pnb[0][0] = NEG_INF; s_last[0][0] = -1; s_len[0][0] = 0; s_node[0][0] = -1;
    s_h[0][0] = CB_H0; s_ph[0][0] = 0;
    if constexpr (LM || BIAS) s_add[0][0] = 0.f;
    if constexpr (BIAS) { s_bm[0][0] = 1u; s_bpsi[0][0] = 0.f; s_bs[0][0] = 0.f; }
    if constexpr (LM) {
      s_lm[0][0] = 0.f;
      s_cx[0][0] = (uint64_t)lm.V;
      int cl = 0;
      for (int k = 0; k < NG_MAXN - 1; ++k) s_bo[0][0][k] = 0.f;
      if (lm.order > 1) {                              // the context is <s>: its backoff, or the OOV mark where it has no unigram
        float lp[NG_MAXN], bo[NG_MAXN];
        const uint32_t f = ng_probe_grams(lm.t, 0, 0, lm.V, lp, bo);
        if (f & 1u) s_bo[0][0][0] = bo[0];
        cl = 1 | ((f & 1u) ? 0 : 1 << 8);
      }
      s_cl[0][0] = cl;
    }
  }
  int cur = 0, n = 1;
  const bool loader = tid < K;                         // K <= 128 < CB_NT
  const int64_t fr0 = (int64_t)b * T * K;
  float nlp = 0.f;
  int ntok = 0;
  if (loader && len > 0) { nlp = top_lp[fr0 + tid]; ntok = top_tok[fr0 + tid]; }
  __syncthreads();
  for (int t = 0; t < len && n > 0; ++t) {
    const int nxt = cur ^ 1;
    if (loader) {
      f_lp[tid] = nlp; f_tok[tid] = ntok;
      if (t + 1 < len) { nlp = top_lp[fr0 + (int64_t)(t + 1) * K + tid]; ntok = top_tok[fr0 + (int64_t)(t + 1) * K + tid]; }   // next frame, in flight during this one
    }
    if (tid == 0) s_n[nxt] = 0;
    __syncthreads();
    // (1) extension scores; an extension naming a string already in the beam is merged into that stay (step 1b)
    for (int e = tid; e < n * K; e += CB_NT) {
      const int i = e / K, c = f_tok[e - i * K];
      float s = NEG_INF;
      if (c != blank) {
        s = (c == s_last[cur][i] ? s_pb[cur][i] : cb_lae(s_pb[cur][i], s_pnb[cur][i])) + f_lp[e - i * K];
        const uint64_t h = s_h[cur][i];
        const int l1 = s_len[cur][i] + 1;
#pragma unroll 8
        for (int j = 0; j < n; ++j)
          if (s_len[cur][j] == l1 && s_last[cur][j] == c && s_ph[cur][j] == h) s = NEG_INF;
        if constexpr (LM) {
          if (s != NEG_INF) {                          // the <= order probes of (context suffix, c), all in flight together
            float lp[NG_MAXN], bo[NG_MAXN];
            const int cl = s_cl[cur][i], L = cl & 0xff;
            const uint32_t f = ng_probe_grams(lm.t, s_cx[cur][i], L, c, lp, bo);
            s += cb_addend(lm, f, lp, s_bo[cur][i], L, (cl >> 8) != 0);
          }
        }
        if constexpr (BIAS) {                          // behind the n-gram's addend: a = psi_minus(state(s c)) - psi(state(s))
          if (s != NEG_INF) s = __fadd_rn(s, __fsub_rn(cb_bias_next(bz, s_bm[cur][i], s_bn[cur][i], c), s_bpsi[cur][i]));
        }
      }
      x_s[e] = CbPair{s, c};
    }
    // (1b) stays: blank, repeat of the last token, and the one extension (parent slot, last token) that names the same string
    if (tid < n) {
      const int j = tid, lj = s_last[cur][j];
      float pbl = NEG_INF, pl = NEG_INF;
#pragma unroll 8
      for (int k = 0; k < K; ++k) {
        if (f_tok[k] == blank) pbl = f_lp[k];
        if (f_tok[k] == lj) pl = f_lp[k];
      }
      const float pb = cb_lae(s_pb[cur][j], s_pnb[cur][j]) + pbl;
      float pnb = s_pnb[cur][j] + pl;
      if (lj >= 0 && pl != NEG_INF) {
        const uint64_t ph = s_ph[cur][j];
        const int l0 = s_len[cur][j] - 1;
#pragma unroll 8
        for (int i = 0; i < n; ++i)
          if (s_len[cur][i] == l0 && s_h[cur][i] == ph) {
            if constexpr (LM || BIAS)                    // the same string: the same addend as when slot j was made
              pnb = cb_lae(pnb, (s_last[cur][i] == lj ? s_pb[cur][i] : cb_lae(s_pb[cur][i], s_pnb[cur][i])) + pl + s_add[cur][j]);
            else
              pnb = cb_lae(pnb, (s_last[cur][i] == lj ? s_pb[cur][i] : cb_lae(s_pb[cur][i], s_pnb[cur][i])) + pl);
          }
      }
      st_pb[j] = pb;
      st_pnb[j] = pnb;
      c_s[j] = CbPair{cb_lae(pb, pnb), j << 16};
    }
    for (int e = n + tid; e < n + n * W; e += CB_NT) c_s[e] = CbPair{NEG_INF, 0};
    __syncthreads();
    // (2) per slot, only its W best extensions can enter the beam: rank them within the slot
    for (int e = tid; e < n * K; e += CB_NT) {
      const float s = x_s[e].s;
      if (s == NEG_INF) continue;
      const int i = e / K, tok = x_s[e].k;
      const CbPair* xi = x_s + i * K;
      int r = 0;
#pragma unroll 8
      for (int k = 0; k < K; ++k) {
        const CbPair o = xi[k];
        r += o.s > s || (o.s == s && o.k < tok);
      }
      if (r < W) c_s[n + i * W + r] = CbPair{s, (i << 16) | (tok + 1)};
    }
    __syncthreads();
    // (3) rank every live candidate among all of them; rank r < W becomes slot r of the next beam
    const int M = n + n * W;
    for (int e = tid; e < M; e += CB_NT) {
      const float s = c_s[e].s;
      if (s == NEG_INF) continue;
      const int key = c_s[e].k;
      int r = 0;
#pragma unroll 8
      for (int q = 0; q < M; ++q) {
        const CbPair o = c_s[q];
        r += cb_better(o.s, o.k, s, key);
      }
      if (r >= W) continue;
      atomicAdd(&s_n[nxt], 1);
      const int i = key >> 16, tp = key & 0xffff;
      if (tp == 0) {
        s_pb[nxt][r] = st_pb[i]; s_pnb[nxt][r] = st_pnb[i];
        s_last[nxt][r] = s_last[cur][i]; s_len[nxt][r] = s_len[cur][i]; s_node[nxt][r] = s_node[cur][i];
        s_h[nxt][r] = s_h[cur][i]; s_ph[nxt][r] = s_ph[cur][i];
        if constexpr (LM) {
          s_cx[nxt][r] = s_cx[cur][i]; s_cl[nxt][r] = s_cl[cur][i]; s_add[nxt][r] = s_add[cur][i]; s_lm[nxt][r] = s_lm[cur][i];
          for (int k = 0; k < NG_MAXN - 1; ++k) s_bo[nxt][r][k] = s_bo[cur][i][k];
        }
        if constexpr (BIAS) {
          if constexpr (!LM) s_add[nxt][r] = s_add[cur][i];
          s_bm[nxt][r] = s_bm[cur][i]; s_bpsi[nxt][r] = s_bpsi[cur][i]; s_bs[nxt][r] = s_bs[cur][i];
          for (int k = 0; k < BS_MAXLEN; ++k) s_bn[nxt][r][k] = s_bn[cur][i][k];
        }
      } else {
        const int c = tp - 1;
        s_pb[nxt][r] = NEG_INF; s_pnb[nxt][r] = s;
        s_last[nxt][r] = c; s_len[nxt][r] = s_len[cur][i] + 1; s_node[nxt][r] = t * W + r;
        s_h[nxt][r] = cb_hash(s_h[cur][i], c); s_ph[nxt][r] = s_h[cur][i];
        tr[t * W + r] = make_int2(s_node[cur][i], c);
        if constexpr (LM) {
          // the probes of step 1 again (the entries are in cache): their log-probs give the addend, their backoffs are those of
          // the new context's suffixes, and a missing unigram marks c as OOV for the slots that will hold it in their window
          float lp[NG_MAXN], bo[NG_MAXN];
          const int cl = s_cl[cur][i], L = cl & 0xff, N1 = lm.order - 1;
          const uint32_t f = ng_probe_grams(lm.t, s_cx[cur][i], L, c, lp, bo);
          const float a = cb_addend(lm, f, lp, s_bo[cur][i], L, (cl >> 8) != 0);
          s_add[nxt][r] = a;
          s_lm[nxt][r] = s_lm[cur][i] + a;
          const int L2 = min(L + 1, N1);
          const uint64_t keep = N1 >= 4 ? ~0ull : (1ull << (16 * N1)) - 1ull;
          s_cx[nxt][r] = ((s_cx[cur][i] << 16) | (uint64_t)(uint32_t)c) & keep;
          const int oov = (((cl >> 8) << 1) | ((f & 1u) ? 0 : 1)) & ((1 << N1) - 1);
          s_cl[nxt][r] = L2 | (oov << 8);
          for (int k = 0; k < NG_MAXN - 1; ++k) s_bo[nxt][r][k] = (k < L2 && (f >> k & 1)) ? bo[k] : 0.f;
        }
        if constexpr (BIAS) {
          // the new chain: child(n_j, c) for every j of the parent's chain below max_len (step 1 just touched the entries); the
          // deepest of them is state(s c), its psi_minus the addend's first term
          const uint32_t pm_mask = s_bm[cur][i] & ((1u << bz.max_len) - 1u);
          uint32_t nm = 1u;
          float pm_new = 0.f, psi_new = 0.f;
          for (int j = 0; j < BS_MAXLEN; ++j) {        // ascending: the deepest hit is the last to set pm_new / psi_new
            if (!(pm_mask >> j & 1u)) continue;
            uint32_t child;
            float pm = 0.f;
            bool end;
            if (bs_child(bz.t, j ? s_bn[cur][i][j - 1] : 0u, (uint32_t)c, child, pm, end)) {
              s_bn[nxt][r][j] = child;                 // depth j + 1 <= 16
              nm |= 2u << j;
              pm_new = pm;
              psi_new = end ? 0.f : pm;
            }
          }
          const float a = __fsub_rn(pm_new, s_bpsi[cur][i]);
          s_bm[nxt][r] = nm; s_bpsi[nxt][r] = psi_new;
          s_bs[nxt][r] = __fadd_rn(s_bs[cur][i], a);
          if constexpr (LM) s_add[nxt][r] = __fadd_rn(s_add[nxt][r], a);   // written just above by this thread: LM, then phrase
          else s_add[nxt][r] = a;
        }
      }
    }
    __syncthreads();
    n = s_n[nxt];
    cur = nxt;
  }
  // BIAS: an open match is refunded -- every live slot loses psi(state(h)) -- and the live slots are ranked again by the refunded
  // score, by counting: descending, ties -> the earlier slot.  s_perm: output row -> slot.
  if constexpr (BIAS) {
    if (tid < n) s_fin[tid] = __fsub_rn(cb_lae(s_pb[cur][tid], s_pnb[cur][tid]), s_bpsi[cur][tid]);
    __syncthreads();
    if (tid < n) {
      const float v = s_fin[tid];
      int r = 0;
      for (int q = 0; q < n; ++q) {
        const float o = s_fin[q];
        r += o > v || (o == v && q < tid);
      }
      s_perm[r] = tid;
    }
    __syncthreads();
  }
  // hypotheses, sorted by score (the last selection ranked them); slots past the live beam: score -inf, length 0, all -1
  int64_t* tk = tokens + (int64_t)b * W * T;
  for (int e = tid; e < W * T; e += CB_NT) {
    const int r = e / T, pos = e - r * T;
    bool pad = r >= n;
    if (!pad) {
      if constexpr (BIAS) pad = pos >= s_len[cur][s_perm[r]];
      else pad = pos >= s_len[cur][r];
    }
    if (pad) tk[e] = -1;
  }
  if (tid < W) {
    const int r = tid;
    const bool live = r < n;
    int src = r;                                       // the slot that output row r shows
    if constexpr (BIAS) src = live ? s_perm[r] : r;
    const int l = live ? s_len[cur][src] : 0;
    if constexpr (BIAS) {
      scores[b * W + r] = live ? s_fin[src] : NEG_INF;
      bz.bias_scores[b * W + r] = live ? __fsub_rn(s_bs[cur][src], s_bpsi[cur][src]) : 0.f;
    } else {
      scores[b * W + r] = live ? cb_lae(s_pb[cur][r], s_pnb[cur][r]) : NEG_INF;
    }
    if constexpr (LM) lm.lm_scores[b * W + r] = live ? s_lm[cur][src] : 0.f;
    out_len[b * W + r] = l;
    int node = live ? s_node[cur][src] : -1;
    for (int pos = l - 1; pos >= 0; --pos) {
      const int2 nd = tr[node];
      tk[(int64_t)r * T + pos] = nd.y;
      node = nd.x;
    }
  }
}

extern "C" int64_t otr_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t W) {
  if (B < 1 || T < 1 || W < 1 || W > CB_MAXW) return -1;
  return (int64_t)B * T * W * (int64_t)sizeof(int2);
}

extern "C" int32_t otr_ctc_topk(const float* log_probs, int64_t ld, const int32_t* lengths, int32_t B, int32_t T, int32_t V,
                                int32_t K, float* top_lp, int32_t* top_tok, void* stream) {
  OTR_REQUIRE(log_probs && lengths && top_lp && top_tok, "ctc_topk: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1, "ctc_topk: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(V >= 1 && V <= CB_MAXV && ld >= V, "ctc_topk: V=%d must be in [1, %d] and ld=%lld >= V", V, CB_MAXV, (long long)ld);
  OTR_REQUIRE(K >= 1 && K <= CB_MAXK && K <= V, "ctc_topk: K=%d must be in [1, min(%d, V=%d)]", K, CB_MAXK, V);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((int64_t)B * T));
  if (V <= 64 * 16)
    hipLaunchKernelGGL(ctc_topk_kernel<16>, grid, dim3(64), 0, s, log_probs, ld, lengths, T, V, K, top_lp, top_tok);
  else if (V <= 64 * 72)
    hipLaunchKernelGGL(ctc_topk_kernel<72>, grid, dim3(64), 0, s, log_probs, ld, lengths, T, V, K, top_lp, top_tok);
  else
    hipLaunchKernelGGL(ctc_topk_kernel<128>, grid, dim3(64), 0, s, log_probs, ld, lengths, T, V, K, top_lp, top_tok);
  return otr_check_launch("ctc_topk");
}

extern "C" int32_t otr_ctc_beam_search(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T,
                                       int32_t V, int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes,
                                       int64_t* tokens, int32_t* out_len, float* scores, void* stream) {
  OTR_REQUIRE(top_lp && top_tok && lengths && workspace && tokens && out_len && scores, "ctc_beam_search: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1, "ctc_beam_search: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(W >= 1 && W <= CB_MAXW, "ctc_beam_search: beam width W=%d must be in [1, %d]", W, CB_MAXW);
  OTR_REQUIRE(V >= 1 && V <= CB_MAXV, "ctc_beam_search: V=%d must be in [1, %d]", V, CB_MAXV);
  OTR_REQUIRE(K >= 1 && K <= CB_MAXK && K <= V, "ctc_beam_search: K=%d must be in [1, min(%d, V=%d)]", K, CB_MAXK, V);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_beam_search: blank=%d must be in [0, V=%d)", blank, V);
  OTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "ctc_beam_search: workspace must be 8-byte aligned");
  const int64_t need = otr_ctc_beam_workspace_bytes(B, T, W);
  OTR_REQUIRE(ws_bytes >= need, "ctc_beam_search: workspace of %lld bytes, %lld needed (otr_ctc_beam_workspace_bytes)",
              (long long)ws_bytes, (long long)need);
  hipLaunchKernelGGL((ctc_beam_search_kernel<false, false>), dim3(B), dim3(CB_NT), 0, (hipStream_t)stream, top_lp, top_tok, lengths, T, K, blank,
                     W, (int2*)workspace, tokens, out_len, scores, CbLm{}, CbBias{});
  return otr_check_launch("ctc_beam_search");
}

extern "C" int32_t otr_ctc_beam_search_lm(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T,
                                          int32_t V, int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes,
                                          int64_t* tokens, int32_t* out_len, float* scores, const void* table, int64_t capacity,
                                          int32_t max_probe, int32_t order, float alpha, float beta, float oov_score,
                                          float* lm_scores, void* stream) {
  OTR_REQUIRE(top_lp && top_tok && lengths && workspace && tokens && out_len && scores && lm_scores, "ctc_beam_search_lm: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1, "ctc_beam_search_lm: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(W >= 1 && W <= CB_MAXW, "ctc_beam_search_lm: beam width W=%d must be in [1, %d]", W, CB_MAXW);
  OTR_REQUIRE(V >= 1 && V <= CB_MAXV, "ctc_beam_search_lm: V=%d must be in [1, %d]", V, CB_MAXV);
  OTR_REQUIRE(K >= 1 && K <= CB_MAXK && K <= V, "ctc_beam_search_lm: K=%d must be in [1, min(%d, V=%d)]", K, CB_MAXK, V);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_beam_search_lm: blank=%d must be in [0, V=%d)", blank, V);
  OTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "ctc_beam_search_lm: workspace must be 8-byte aligned");
  const int64_t need = otr_ctc_beam_workspace_bytes(B, T, W);
  OTR_REQUIRE(ws_bytes >= need, "ctc_beam_search_lm: workspace of %lld bytes, %lld needed (otr_ctc_beam_workspace_bytes)",
              (long long)ws_bytes, (long long)need);
  if (otr_ngram_check_table("ctc_beam_search_lm", table, capacity, max_probe, order, V) < 0) return -1;
  OTR_REQUIRE(alpha == alpha && beta == beta && oov_score == oov_score, "ctc_beam_search_lm: alpha, beta and oov_score must be numbers");
  const CbLm lm{NgTable{(const uint4*)table, (uint32_t)(capacity - 1), max_probe}, order, V, alpha, beta, oov_score, lm_scores};
  hipLaunchKernelGGL((ctc_beam_search_kernel<true, false>), dim3(B), dim3(CB_NT), 0, (hipStream_t)stream, top_lp, top_tok, lengths, T, K, blank,
                     W, (int2*)workspace, tokens, out_len, scores, lm, CbBias{});
  return otr_check_launch("ctc_beam_search_lm");
}

extern "C" int32_t otr_ctc_beam_search_bias(const float* top_lp, const int32_t* top_tok, const int32_t* lengths, int32_t B, int32_t T,
                                            int32_t V, int32_t K, int32_t blank, int32_t W, void* workspace, int64_t ws_bytes,
                                            int64_t* tokens, int32_t* out_len, float* scores, const void* ngram_table, int64_t capacity,
                                            int32_t max_probe, int32_t order, float alpha, float beta, float oov_score, float* lm_scores,
                                            const void* bias_table, int64_t bias_capacity, int32_t bias_max_probe, int32_t bias_max_len,
                                            float* bias_scores, void* stream) {
  OTR_REQUIRE(top_lp && top_tok && lengths && workspace && tokens && out_len && scores && bias_scores, "ctc_beam_search_bias: null pointer");
  OTR_REQUIRE(B >= 1 && T >= 1, "ctc_beam_search_bias: bad shape B=%d T=%d", B, T);
  OTR_REQUIRE(W >= 1 && W <= CB_MAXW, "ctc_beam_search_bias: beam width W=%d must be in [1, %d]", W, CB_MAXW);
  OTR_REQUIRE(V >= 1 && V <= CB_MAXV, "ctc_beam_search_bias: V=%d must be in [1, %d]", V, CB_MAXV);
  OTR_REQUIRE(K >= 1 && K <= CB_MAXK && K <= V, "ctc_beam_search_bias: K=%d must be in [1, min(%d, V=%d)]", K, CB_MAXK, V);
  OTR_REQUIRE(blank >= 0 && blank < V, "ctc_beam_search_bias: blank=%d must be in [0, V=%d)", blank, V);
  OTR_REQUIRE(((uintptr_t)workspace & 7) == 0, "ctc_beam_search_bias: workspace must be 8-byte aligned");
  const int64_t need = otr_ctc_beam_workspace_bytes(B, T, W);
  OTR_REQUIRE(ws_bytes >= need, "ctc_beam_search_bias: workspace of %lld bytes, %lld needed (otr_ctc_beam_workspace_bytes)",
              (long long)ws_bytes, (long long)need);
  if (otr_bias_check_table("ctc_beam_search_bias", bias_table, bias_capacity, bias_max_probe, bias_max_len) < 0) return -1;
  const CbBias bz{BsTable{(const uint4*)bias_table, (uint32_t)(bias_capacity - 1), bias_max_probe}, bias_max_len, bias_scores};
  hipStream_t s = (hipStream_t)stream;
  if (!ngram_table) {                                  // no n-gram: its arguments are not looked at, lm_scores must not be given
    OTR_REQUIRE(lm_scores == nullptr, "ctc_beam_search_bias: lm_scores given without an n-gram table");
    hipLaunchKernelGGL((ctc_beam_search_kernel<false, true>), dim3(B), dim3(CB_NT), 0, s, top_lp, top_tok, lengths, T, K, blank, W,
                       (int2*)workspace, tokens, out_len, scores, CbLm{}, bz);
    return otr_check_launch("ctc_beam_search_bias");
  }
  OTR_REQUIRE(lm_scores != nullptr, "ctc_beam_search_bias: null lm_scores with an n-gram table");
  if (otr_ngram_check_table("ctc_beam_search_bias", ngram_table, capacity, max_probe, order, V) < 0) return -1;
  OTR_REQUIRE(alpha == alpha && beta == beta && oov_score == oov_score, "ctc_beam_search_bias: alpha, beta and oov_score must be numbers");
  const CbLm lm{NgTable{(const uint4*)ngram_table, (uint32_t)(capacity - 1), max_probe}, order, V, alpha, beta, oov_score, lm_scores};
  hipLaunchKernelGGL((ctc_beam_search_kernel<true, true>), dim3(B), dim3(CB_NT), 0, s, top_lp, top_tok, lengths, T, K, blank, W,
                     (int2*)workspace, tokens, out_len, scores, lm, bz);
  return otr_check_launch("ctc_beam_search_bias");
}
