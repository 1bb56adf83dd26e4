// One wave's logsumexp of one row of f32 logits, read once: every lane keeps a running maximum and a sum of exp(x - max) of what it has
// seen, the wave combines them at the end.  Shared by the teacher-forced scorers (rescore.hip: otr_rescore_score; mwer.hip: otr_mwer_loss)
// so that both form a row's log-softmax with the same arithmetic.
#pragma once
#include "common.h"

#ifndef NEG_INF
#define NEG_INF (-__builtin_huge_valf())
#endif

struct RsRun { float m, s; };      // running maximum and sum of exp(x - m) of what a lane has seen (m = -inf: nothing finite yet, s = 0)

__device__ __forceinline__ void rs_take(RsRun& r, float x) {
  if (x > r.m) {                                      // new maximum: rescale (exp(-inf - x) = 0 the first time)
    r.s = r.s * __expf(r.m - x) + 1.f;
    r.m = x;
  } else if (x > NEG_INF) {
    r.s += __expf(x - r.m);
  }
}
__device__ __forceinline__ void rs_take4(RsRun& r, const float4& q) {
  const float mq = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  if (mq > r.m) {
    r.s *= __expf(r.m - mq);
    r.m = mq;
  }
  if (r.m > NEG_INF) r.s += __expf(q.x - r.m) + __expf(q.y - r.m) + __expf(q.z - r.m) + __expf(q.w - r.m);
}

// the row x[0 .. V) by the 64 lanes of a wave: M = its maximum, S = sum of exp(x - M), on every lane.  vec: x is 16-byte aligned
// (the caller checked the base and the row stride), so the row is read with 16-byte loads, four in flight per lane.
__device__ __forceinline__ void rs_row(const float* x, int V, bool vec, int lane, float& M, float& S) {
  RsRun r{NEG_INF, 0.f};
  if (vec) {
    const int nq = V >> 2;
    int q = lane;
    for (; q + 192 < nq; q += 256) {                // four loads in flight per lane
      const float4 a = *reinterpret_cast<const float4*>(x + 4 * q);
      const float4 b = *reinterpret_cast<const float4*>(x + 4 * (q + 64));
      const float4 c = *reinterpret_cast<const float4*>(x + 4 * (q + 128));
      const float4 d = *reinterpret_cast<const float4*>(x + 4 * (q + 192));
      rs_take4(r, a); rs_take4(r, b); rs_take4(r, c); rs_take4(r, d);
    }
    for (; q < nq; q += 64) rs_take4(r, *reinterpret_cast<const float4*>(x + 4 * q));
    for (int v = 4 * nq + lane; v < V; v += 64) rs_take(r, x[v]);    // the row's last, partial quad
  } else {
    for (int v = lane; v < V; v += 64) rs_take(r, x[v]);
  }
  M = wave_max(r.m);
  S = wave_sum(r.m > NEG_INF ? r.s * __expf(r.m - M) : 0.f);
}
