// Device helpers shared by the gated-attention MIL kernels (attmil.hip, chowder.hip, clam.hip,
// dtfd.hip); include after common.h.  Every reduction here has one fixed combination order, so the
// kernels that use them repeat bitwise.
#pragma once
#include <limits.h>

TM_DEV float sigmoid_(float x) { return 1.f / (1.f + expf(-x)); }
// the hardware-exp form (attmil.hip only): different bits from sigmoid_, never a stand-in for it
TM_DEV float sigmoid_fast(float x) { return 1.f / (1.f + __expf(-x)); }

TM_DEV float dot4(f32x4 a, f32x4 b, float acc) {
#pragma unroll
  for (int u = 0; u < 4; ++u) acc = fmaf(a[u], b[u], acc);
  return acc;
}

// Block-wide sum / max of one value per thread: the wave butterfly, then waves 0..nw-1 in order
// (red: one float per wave).  NWAVES: the workgroup's wave count where the kernel fixes it (the loop
// is then unrolled), 0: blockDim.x >> 6.
template <bool MAX, int NWAVES = 0>
TM_DEV float block_reduce(float v, float* red) {
  v = MAX ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  if constexpr (NWAVES > 0) {
#pragma unroll
    for (int i = 1; i < NWAVES; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
  } else {
    for (int i = 1; i < nw; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
  }
  return r;
}

// log-sum-exp of C values, max-shifted
TM_DEV float lse_of(const float* v, int C) {
  float mx = v[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, v[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(v[c] - mx);
  return mx + logf(s);
}

// The gate g = tanh(za) * sigmoid(zb) and its backward: from dg = d loss / d g and the saved
// th = tanh(za), sg = sigmoid(zb), the gradients of za and zb.
TM_DEV float gate(float za, float zb) { return tanhf(za) * sigmoid_(zb); }
TM_DEV f32x4 gate(const f32x4& za, const f32x4& zb) {
  f32x4 g;
#pragma unroll
  for (int u = 0; u < 4; ++u) g[u] = tanhf(za[u]) * sigmoid_(zb[u]);
  return g;
}
struct GateGrad {
  float a, b;
};
TM_DEV GateGrad gate_bwd(float dg, float th, float sg) {
  return {dg * sg * (1.f - th * th), dg * th * sg * (1.f - sg)};
}

// Typed rows (T = float or bf16 storage, fp32 arithmetic): 8 consecutive elements of a row as
// floats and back (bf16: one 16-byte access; fp32: two).  p must be 16-B aligned.
template <typename T>
TM_DEV f32x8 load8f(const T* p) {
  const vec8<T> v = load8<T>(p);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = to_f(v[e]);
  return r;
}
template <typename T>
TM_DEV void store8f(T* p, const f32x8& x) {
  vec8<T> v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = from_f<T>(x[e]);
  store8<T>(p, v);
}
TM_DEV float dot8(const f32x8& a, const f32x8& b, float acc) {
#pragma unroll
  for (int u = 0; u < 8; ++u) acc = fmaf(a[u], b[u], acc);
  return acc;
}
// th = tanh(za), sg = sigmoid(zb) of 8 gate inputs; the gate itself is th * sg
TM_DEV void gate_parts8(const f32x8& za, const f32x8& zb, f32x8& th, f32x8& sg) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    th[u] = tanhf(za[u]);
    sg[u] = sigmoid_(zb[u]);
  }
}

// Two-sided selection: (score, instance index) pairs in ascending-score order (before_min) and in
// descending-score order (before_max); among equal scores the lower index comes first in both.
struct Pair {
  float v;
  int i;
};
TM_DEV bool before_min(float v, int i, Pair p) { return v < p.v || (v == p.v && i < p.i); }
TM_DEV bool before_max(float v, int i, Pair p) { return v > p.v || (v == p.v && i < p.i); }

template <bool MAXSIDE>
TM_DEV Pair wave_first(Pair p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(p.v, o, 64);
    const int i = __shfl_xor(p.i, o, 64);
    if (MAXSIDE ? before_max(v, i, p) : before_min(v, i, p)) p = {v, i};
  }
  return p;
}

// The tail of one selection round: from every thread's candidates (lo: its first pair in ascending
// order, hi: in descending order) to the workgroup's, in every thread.  The wave butterfly, the
// hand-off through q [2][NWAVES] (LDS), then waves 0..NWAVES-1 in order.  One barrier: the caller
// alternates between two buffers from round to round, so no wave can overwrite what another still reads.
struct PairLoHi {
  Pair lo, hi;
};
template <int NWAVES>
TM_DEV PairLoHi select_round_tail(Pair lo, Pair hi, Pair (*q)[NWAVES]) {
  lo = wave_first<false>(lo);
  hi = wave_first<true>(hi);
  if ((threadIdx.x & 63) == 0) {
    q[0][threadIdx.x >> 6] = lo;
    q[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  lo = q[0][0];
  hi = q[1][0];
#pragma unroll
  for (int u = 1; u < NWAVES; ++u) {
    const Pair a = q[0][u], c = q[1][u];
    if (before_min(a.v, a.i, lo)) lo = a;
    if (before_max(c.v, c.i, hi)) hi = c;
  }
  return {lo, hi};
}
// a selected index, in [0, N) whatever the scores were (NaN / Inf input)
TM_DEV int select_clamp(int i, int N) { return min(max(i, 0), N - 1); }
