// Geometry-generic NystromAttention core in fp32 (the tm_nysg_* family): the same maths as the
// parity path (nystrom_f32.h, pinv.hip) for the TransMIL widths other than 512,
//   (dim_head, landmarks) = (32, 128)   out_features = 256
//                           (48, 192)   out_features = 384
// TransLayer always builds dim_head = dim / 8 and landmarks = dim / 2 (code/models/TransMIL.py:26-31),
// so NL == 4 DH in every geometry; the kernels below lean on that: a workgroup has NL threads,
// thread = key in the score phases and (query of a 16-query chunk, 4 consecutive d) in the
// product phases (16 * DH / 4 == NL items).  fp32 FMA arithmetic and fp32 accumulation throughout;
// every operand and result is fp32 except the dqkv the assemble pass writes in the GEMM dtype.
// (48, 192) is not a power of two: no index below is split by shifts or masks of DH / NL, waves
// per workgroup are NL / 64 = 2 or 3, and every global access is a 16-B piece of a DH-float row
// (DH * 4 bytes is a multiple of 16).
//
// Layouts (bh = bag * heads + head, n = padded length, a multiple of NL; l = n / NL):
//   q, k, v   [B*h][n][DH]    (q pre-scaled by dim_head^-0.5)
//   ql, kl, W, Y and their gradients  [B*h][NL][DH];  A2, Z and the chain's matrices [B*h][NL][NL]
//   merged, dmerged  [B][n][h*DH]
// Kernels
//   landmarks_g        segment means of q, k
//   a3_fwd_g + a3_combine_g   W = softmax(ql k^T) v per NL-key block, merged in block order; lse3
//   softmax_rows_g     A2 = softmax over rows of the ql kl^T logits (tm_bmm), in place
//   pinv_*_g           abs-sum maxima over ALL bags and heads, Z0, Z0's backward (the chain's
//                      products are tm_bmm jobs, exact fp32)
//   mm_g               [NL x NL] (or its transpose) times [NL x DH] (+ addend): Y, dW, dq~, dk~
//   a1_fwd_g           softmax(q kl^T) Y + conv33(v) -> merged rows, lse1
//   conv_bwd_g         conv33 backward, D1, dwconv partials
//   attn_bwd_g<MODE>   flash-style backward of the A1 / A3 products
//   softmax_bwd_rows_g, assemble_dqkv_g, attn_row_g
// Determinism: no float atomics, every sum in a fixed order, no host sync, no allocation.
#include <algorithm>
#include "common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int TAPS = 33;   // residual conv kernel
constexpr int HALF = 16;   // conv padding
constexpr int QC = 16;     // queries per chunk
constexpr int QPW = 64;    // queries per workgroup of the two forward products
constexpr int CB_R = 32;   // rows per workgroup of the conv backward

inline bool geo_ok(int dh, int nl) { return (dh == 32 && nl == 128) || (dh == 48 && nl == 192); }
#define TM_GEO_MSG "nysg: (dh, nl) must be (32, 128) or (48, 192)"
#define TM_GEO_REQUIRE(dh, nl) TM_REQUIRE(geo_ok(dh, nl), TM_GEO_MSG)
#define TM_GEO_DISPATCH(dh, CALL)                           \
  if ((dh) == 32) { constexpr int DH = 32, NL = 128; CALL; } \
  else { constexpr int DH = 48, NL = 192; CALL; }
#define TM_NL_DISPATCH(nl, CALL)               \
  if ((nl) == 128) { constexpr int NL = 128; CALL; } \
  else { constexpr int NL = 192; CALL; }

TM_DEV void fma4(f32x4& acc, float a, const f32x4& b) {
  acc[0] = fmaf(a, b[0], acc[0]); acc[1] = fmaf(a, b[1], acc[1]);
  acc[2] = fmaf(a, b[2], acc[2]); acc[3] = fmaf(a, b[3], acc[3]);
}

// ---------------------------------------------------------------------------
// landmarks: out[row][d] = sum_{t<l} x[row * l + t][d] / l with row = bh * NL + j (bh * n + j * l ==
// row * l); grid (ceil(rows * DH / 4 / 256), 2: q / k), block 256, thread = (row, 4 d)
template <int DH>
__global__ __launch_bounds__(256) void landmarks_g(const float* __restrict__ q, const float* __restrict__ k,
                                                   long long rows, int l, float* __restrict__ ql,
                                                   float* __restrict__ kl) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= rows * (DH / 4)) return;
  const long long row = item / (DH / 4);
  const int d4 = (int)(item % (DH / 4)) * 4;
  const float* src = (blockIdx.y ? k : q) + (size_t)row * l * DH + d4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < l; ++t) s += *(const f32x4*)(src + (size_t)t * DH);
  const float fl = (float)l;
  *(f32x4*)((blockIdx.y ? kl : ql) + (size_t)row * DH + d4) = s / fl;
}

// ---------------------------------------------------------------------------
// Shared forward chunk: NL threads, thread = key (its key row in registers), QC queries in LDS.
// Leaves p = exp(s - max) in ps[q][key] and the per-wave max / sum in red[0 / 1][wave][q].
template <int DH, int NL>
TM_DEV void fwd_chunk(const float (&kreg)[DH], const float* qs, float* ps, float* red, int tid) {
  constexpr int NW = NL / 64;
  const int wave = tid >> 6, lane = tid & 63;
  // the logits pass through ps (rolled loops over the queries: holding all QC logits and their
  // query pieces in registers spilled to scratch)
#pragma unroll 1
  for (int qi = 0; qi < QC; ++qi) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const f32x4 q4 = *(const f32x4*)(qs + qi * DH + d);
      s = fmaf(q4[0], kreg[d], s); s = fmaf(q4[1], kreg[d + 1], s);
      s = fmaf(q4[2], kreg[d + 2], s); s = fmaf(q4[3], kreg[d + 3], s);
    }
    ps[qi * (NL + 4) + tid] = s;
    const float m = wave_max_dpp(s);
    if (lane == 0) red[wave * QC + qi] = m;
  }
  __syncthreads();
#pragma unroll 1
  for (int qi = 0; qi < QC; ++qi) {
    float m = red[qi];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w * QC + qi]);
    const float p = __expf(ps[qi * (NL + 4) + tid] - m);
    ps[qi * (NL + 4) + tid] = p;
    const float t = wave_sum_dpp(p);
    if (lane == 0) red[(NW + wave) * QC + qi] = t;
  }
  __syncthreads();
}

// the (query, 4 d) item of the product phase: max, sum and the unnormalised p . V row piece
template <int DH, int NL>
TM_DEV f32x4 fwd_item(const float* ps, const float* vs, const float* red, int qi, int d4, float& M, float& L) {
  constexpr int NW = NL / 64;
  M = red[qi];
  L = red[NW * QC + qi];
#pragma unroll
  for (int w = 1; w < NW; ++w) { M = fmaxf(M, red[w * QC + qi]); L += red[(NW + w) * QC + qi]; }
  // four interleaved partial sums (keys 4j + i), combined pairwise: chains of NL / 4 terms
  f32x4 acc[4] = {};
#pragma unroll 4
  for (int key = 0; key < NL; key += 4) {
    const f32x4 p4 = *(const f32x4*)(ps + qi * (NL + 4) + key);
#pragma unroll
    for (int i = 0; i < 4; ++i) fma4(acc[i], p4[i], *(const f32x4*)(vs + (key + i) * DH + d4));
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// ---------------------------------------------------------------------------
// A1 forward.  grid (n / QPW, nbh), block NL.
//   merged[bag][t][head*DH+d] = softmax_j(q_t . kl_j) . Y_j + sum_tau w[head][tau] v[t+tau-16][d]
template <int DH, int NL>
__global__ __launch_bounds__(NL) void a1_fwd_g(const float* __restrict__ q, const float* __restrict__ v,
                                               const float* __restrict__ kl, const float* __restrict__ y,
                                               const float* __restrict__ wconv, int n, int nh,
                                               float* __restrict__ merged, float* __restrict__ lse1) {
  static_assert(NL == QC * DH / 4 && NL % 64 == 0, "thread = (query, 4 d) needs NL == 4 DH");
  constexpr int NW = NL / 64, P4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float vs[NL * DH];
  __shared__ __attribute__((aligned(16))) float qs[QC * DH];
  __shared__ __attribute__((aligned(16))) float ps[QC * (NL + 4)];
  __shared__ __attribute__((aligned(16))) float vw[(QC + 2 * HALF) * DH];
  __shared__ float red[2 * NW * QC];
  __shared__ float ws[TAPS];
  const int tid = threadIdx.x, bh = blockIdx.y, head = bh % nh, bag = bh / nh;
  const int qi = tid / P4, d4 = (tid % P4) * 4;
  const float* yb = y + (size_t)bh * NL * DH;
  float kreg[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const f32x4 t = *(const f32x4*)(kl + ((size_t)bh * NL + tid) * DH + d);
    kreg[d] = t[0]; kreg[d + 1] = t[1]; kreg[d + 2] = t[2]; kreg[d + 3] = t[3];
  }
  for (int c = tid; c < NL * P4; c += NL) *(f32x4*)(vs + c * 4) = *(const f32x4*)(yb + (size_t)c * 4);
  if (tid < TAPS) ws[tid] = wconv[head * TAPS + tid];
  const float* qb = q + (size_t)bh * n * DH;
  const float* vb = v + (size_t)bh * n * DH;
#pragma unroll 1
  for (int c0 = 0; c0 < QPW; c0 += QC) {
    const int qa = blockIdx.x * QPW + c0;
    __syncthreads();   // previous chunk consumed (first pass: nothing pending)
    *(f32x4*)(qs + qi * DH + d4) = *(const f32x4*)(qb + (size_t)(qa + qi) * DH + d4);
#pragma unroll
    for (int i = 0; i < (QC + 2 * HALF) / QC; ++i) {   // the conv window: rows qa - 16 .. qa + 31
      const int row = qi + QC * i, t = qa - HALF + row;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < n) x = *(const f32x4*)(vb + (size_t)t * DH + d4);
      *(f32x4*)(vw + row * DH + d4) = x;
    }
    __syncthreads();
    fwd_chunk<DH, NL>(kreg, qs, ps, red, tid);
    float M, L;
    f32x4 o = fwd_item<DH, NL>(ps, vs, red, qi, d4, M, L) / L;
#pragma unroll
    for (int tau = 0; tau < TAPS; ++tau) fma4(o, ws[tau], *(const f32x4*)(vw + (qi + tau) * DH + d4));
    const int t = qa + qi;
    *(f32x4*)(merged + (((size_t)bag * n + t) * nh + head) * DH + d4) = o;
    if (d4 == 0) lse1[(size_t)bh * n + t] = M + __logf(L);
  }
}

// ---------------------------------------------------------------------------
// A3 forward, one NL-key block x QPW landmark queries per workgroup.  grid (n / NL, nbh, NL / QPW).
//   part_o[kb][bh][q][d] = sum_{keys in kb} exp(s - m_kb) v ; part_m / part_l [kb][bh][q]
template <int DH, int NL>
__global__ __launch_bounds__(NL) void a3_fwd_g(const float* __restrict__ ql, const float* __restrict__ k,
                                               const float* __restrict__ v, int n, float* __restrict__ part_o,
                                               float* __restrict__ part_m, float* __restrict__ part_l) {
  static_assert(NL == QC * DH / 4 && NL % QPW == 0, "thread = (query, 4 d) needs NL == 4 DH");
  constexpr int NW = NL / 64, P4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float vs[NL * DH];
  __shared__ __attribute__((aligned(16))) float qs[QC * DH];
  __shared__ __attribute__((aligned(16))) float ps[QC * (NL + 4)];
  __shared__ float red[2 * NW * QC];
  const int tid = threadIdx.x, kb = blockIdx.x, bh = blockIdx.y, nbh = gridDim.y;
  const int qi = tid / P4, d4 = (tid % P4) * 4;
  const size_t kv = ((size_t)bh * n + (size_t)kb * NL) * DH;
  float kreg[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const f32x4 t = *(const f32x4*)(k + kv + (size_t)tid * DH + d);
    kreg[d] = t[0]; kreg[d + 1] = t[1]; kreg[d + 2] = t[2]; kreg[d + 3] = t[3];
  }
  for (int c = tid; c < NL * P4; c += NL) *(f32x4*)(vs + c * 4) = *(const f32x4*)(v + kv + (size_t)c * 4);
#pragma unroll 1
  for (int c0 = 0; c0 < QPW; c0 += QC) {
    const int qa = blockIdx.z * QPW + c0;
    __syncthreads();
    *(f32x4*)(qs + qi * DH + d4) = *(const f32x4*)(ql + ((size_t)bh * NL + qa + qi) * DH + d4);
    __syncthreads();
    fwd_chunk<DH, NL>(kreg, qs, ps, red, tid);
    float M, L;
    const f32x4 o = fwd_item<DH, NL>(ps, vs, red, qi, d4, M, L);
    const size_t pidx = ((size_t)kb * nbh + bh) * NL + qa + qi;
    *(f32x4*)(part_o + pidx * DH + d4) = o;
    if (d4 == 0) { part_m[pidx] = M; part_l[pidx] = L; }
  }
}

// W[bh][q][d], lse3[bh][q] from the key-block partials, block order; thread = (bh * NL + q, 4 d)
template <int DH, int NL>
__global__ __launch_bounds__(256) void a3_combine_g(const float* __restrict__ part_o, const float* __restrict__ part_m,
                                                    const float* __restrict__ part_l, int nkb, int nbh,
                                                    float* __restrict__ w, float* __restrict__ lse3) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long rows = (long long)nbh * NL;
  if (item >= rows * (DH / 4)) return;
  const size_t row = (size_t)(item / (DH / 4));
  const int d4 = (int)(item % (DH / 4)) * 4;
  float M = -INFINITY;
  for (int kb = 0; kb < nkb; ++kb) M = fmaxf(M, part_m[(size_t)kb * rows + row]);
  float L = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nkb; ++kb) {
    const size_t pidx = (size_t)kb * rows + row;
    const float sc = __expf(part_m[pidx] - M);
    L += part_l[pidx] * sc;
    acc += *(const f32x4*)(part_o + pidx * DH + d4) * sc;
  }
  *(f32x4*)(w + row * DH + d4) = acc / L;
  if (d4 == 0) lse3[row] = M + __logf(L);
}

// ---------------------------------------------------------------------------
// row softmax in place, rows of length NL: one wave per row, grid ceil(rows / 4), block 256
template <int NL>
__global__ __launch_bounds__(256) void softmax_rows_g(float* __restrict__ a, long long rows) {
  constexpr int E = NL / 64;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float* p = a + (size_t)r * NL;
  float x[E];
#pragma unroll
  for (int i = 0; i < E; ++i) x[i] = p[lane + 64 * i];
  float m = x[0];
#pragma unroll
  for (int i = 1; i < E; ++i) m = fmaxf(m, x[i]);
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) { x[i] = __expf(x[i] - m); s += x[i]; }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < E; ++i) p[lane + 64 * i] = x[i] / s;
}

// dS = A * (dA - rowsum(dA * A)), rows of length NL: one wave per row
template <int NL>
__global__ __launch_bounds__(256) void softmax_bwd_rows_g(const float* __restrict__ a, const float* __restrict__ da,
                                                          float* __restrict__ ds, long long rows) {
  constexpr int E = NL / 64;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float av[E], dv[E];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    av[i] = a[(size_t)r * NL + lane + 64 * i];
    dv[i] = da[(size_t)r * NL + lane + 64 * i];
    s = fmaf(av[i], dv[i], s);
  }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < E; ++i) ds[(size_t)r * NL + lane + 64 * i] = av[i] * (dv[i] - s);
}

// ---------------------------------------------------------------------------
// C[bh] = op(A[bh]) B[bh] + e1 E1[bh]; A [NL][NL] (TA: read transposed), B, C, E1 [NL][DH].
// grid (NL / QC, nbh), block NL: QC rows of C per workgroup, thread = (row, 4 d), k in index order.
template <int DH, int NL, int TA>
__global__ __launch_bounds__(NL) void mm_g(const float* __restrict__ A, const float* __restrict__ B,
                                           const float* __restrict__ E1, float e1, float* __restrict__ C) {
  static_assert(NL == QC * DH / 4, "thread = (row, 4 d) needs NL == 4 DH");
  constexpr int P4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float bs[NL * DH];
  __shared__ __attribute__((aligned(16))) float as[QC * (NL + 4)];
  const int tid = threadIdx.x, bh = blockIdx.y, r0 = blockIdx.x * QC;
  const float* a = A + (size_t)bh * NL * NL;
  const float* b = B + (size_t)bh * NL * DH;
  for (int c = tid; c < NL * P4; c += NL) *(f32x4*)(bs + c * 4) = *(const f32x4*)(b + (size_t)c * 4);
  if (TA == 0) {
    for (int c = tid; c < QC * NL / 4; c += NL) {
      const int r = c / (NL / 4), k4 = (c % (NL / 4)) * 4;
      *(f32x4*)(as + r * (NL + 4) + k4) = *(const f32x4*)(a + (size_t)(r0 + r) * NL + k4);
    }
  } else {
#pragma unroll
    for (int r4 = 0; r4 < QC; r4 += 4) {   // thread = k: A[k][r0 .. r0 + 15]
      const f32x4 t = *(const f32x4*)(a + (size_t)tid * NL + r0 + r4);
#pragma unroll
      for (int e = 0; e < 4; ++e) as[(r4 + e) * (NL + 4) + tid] = t[e];
    }
  }
  __syncthreads();
  const int r = tid / P4, d4 = (tid % P4) * 4;
  f32x4 part[4] = {};   // four interleaved partial sums, combined pairwise
#pragma unroll 4
  for (int k = 0; k < NL; k += 4) {
    const f32x4 a4 = *(const f32x4*)(as + r * (NL + 4) + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) fma4(part[i], a4[i], *(const f32x4*)(bs + (k + i) * DH + d4));
  }
  f32x4 acc = (part[0] + part[1]) + (part[2] + part[3]);
  const size_t off = ((size_t)bh * NL + r0 + r) * DH + d4;
  if (E1) acc += *(const f32x4*)(E1 + off) * e1;
  *(f32x4*)(C + off) = acc;
}

// ---------------------------------------------------------------------------
// conv33 backward + D1.  grid (n / CB_R, nbh), block 256.
//   dv[bh][t][d]  = sum_tau w[tau] dO[t - tau + 16][d]
//   c_tau(t)      = sum_d dO[t][d] v[t + tau - 16][d]
//   D1[bh][t]     = dO[t].O[t] - sum_tau w[tau] c_tau(t)          (= dO . (attn1 Y))
//   dw_part[bag*ntb + tb][head*33 + tau] = sum_{t in block} c_tau(t)
template <int DH>
__global__ __launch_bounds__(256) void conv_bwd_g(const float* __restrict__ dmerged, const float* __restrict__ merged,
                                                  const float* __restrict__ v, const float* __restrict__ wconv, int n,
                                                  int nh, float* __restrict__ dv, float* __restrict__ d1,
                                                  float* __restrict__ dw_part) {
  constexpr int R = CB_R, HR = R + 2 * HALF, RW = DH + 4, P4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float dos[HR * RW];
  __shared__ __attribute__((aligned(16))) float vs[HR * RW];
  __shared__ float cred[R][TAPS + 1];
  __shared__ float ws[TAPS];
  const int bh = blockIdx.y, tb = blockIdx.x, tid = threadIdx.x;
  const int head = bh % nh, bag = bh / nh, ntb = gridDim.x, t0 = tb * R, ld = nh * DH;
  const float* dob = dmerged + (size_t)bag * n * ld + head * DH;
  const float* ob = merged + (size_t)bag * n * ld + head * DH;
  const float* vb = v + (size_t)bh * n * DH;
  for (int it = tid; it < HR * P4; it += 256) {
    const int rr = it / P4, d4 = (it % P4) * 4, t = t0 - HALF + rr;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < n) {
      a = *(const f32x4*)(dob + (size_t)t * ld + d4);
      b = *(const f32x4*)(vb + (size_t)t * DH + d4);
    }
    *(f32x4*)(dos + rr * RW + d4) = a;
    *(f32x4*)(vs + rr * RW + d4) = b;
  }
  if (tid < TAPS) ws[tid] = wconv[head * TAPS + tid];
  __syncthreads();
  for (int it = tid; it < R * TAPS; it += 256) {
    const int rl = it / TAPS, tau = it % TAPS;
    float c = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const f32x4 g = *(const f32x4*)(dos + (rl + HALF) * RW + d), x = *(const f32x4*)(vs + (rl + tau) * RW + d);
      c = fmaf(g[0], x[0], c); c = fmaf(g[1], x[1], c); c = fmaf(g[2], x[2], c); c = fmaf(g[3], x[3], c);
    }
    cred[rl][tau] = c;
  }
  __syncthreads();
  if (tid < R) {
    const int t = t0 + tid;   // n is a multiple of R: every row of the block is a token
    float dd = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const f32x4 g = *(const f32x4*)(dos + (tid + HALF) * RW + d), o = *(const f32x4*)(ob + (size_t)t * ld + d);
      dd = fmaf(g[0], o[0], dd); dd = fmaf(g[1], o[1], dd); dd = fmaf(g[2], o[2], dd); dd = fmaf(g[3], o[3], dd);
    }
    float wc = 0.f;
    for (int tau = 0; tau < TAPS; ++tau) wc = fmaf(ws[tau], cred[tid][tau], wc);
    d1[(size_t)bh * n + t] = dd - wc;
  } else if (tid >= 64 && tid < 64 + TAPS) {
    const int tau = tid - 64;
    float sum = 0.f;
    for (int rl = 0; rl < R; ++rl) sum += cred[rl][tau];
    dw_part[((size_t)bag * ntb + tb) * (nh * TAPS) + head * TAPS + tau] = sum;
  }
  for (int it = tid; it < R * P4; it += 256) {
    const int rl = it / P4, d4 = (it % P4) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tau = 0; tau < TAPS; ++tau) fma4(acc, ws[tau], *(const f32x4*)(dos + (rl + 2 * HALF - tau) * RW + d4));
    *(f32x4*)(dv + ((size_t)bh * n + t0 + rl) * DH + d4) = acc;
  }
}

// ---------------------------------------------------------------------------
// Flash-style backward of both attention products.  A workgroup owns NL keys (thread = key: its
// K and V rows and its dK, dV rows stay in registers) and walks queries in chunks of QC.  With
// P = exp(Q K^T - lse), dS = P (dO V^T - D):
//   dV += P^T dO,  dK += dS^T Q   (registers, queries in index order)
//   dQ  = dS K                    (per chunk, dS through LDS; thread = (query, 4 d))
// GB_A1: keys = the NL landmarks, queries = rows [blk * NL, (blk + 1) * NL), D = d1 (conv backward);
//        dQ -> dq (=), dK / dV -> partial slabs [blk].
// GB_A3: keys = k rows of block blk, queries = the NL landmarks, D = rowsum(dO o O) computed here;
//        dK -> dk (=), dV -> dv (+=: it holds the conv backward's dv), dQ -> partial slab [blk].
enum { GB_A3 = 0, GB_A1 = 1 };
struct GBwdArgs {
  const float* q; long long q_bag, q_head; int q_row;
  const float* dO; long long o_bag, o_head; int o_row;
  const float* k; const float* v; long long kv_bh;
  const float* lse; const float* dd; long long lq_bh;
  const float* o;                       // GB_A3: O rows [bh][NL][DH]
  float* dq; long long dq_bh, dq_slab;
  float* dk; float* dv; long long dkv_bh, dkv_slab;
  int nh;
};

template <int DH, int NL, int MODE>
__global__ __launch_bounds__(NL) void attn_bwd_g(GBwdArgs a) {
  static_assert(NL == QC * DH / 4, "thread = (query, 4 d) needs NL == 4 DH");
  constexpr int P4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float ks[NL * DH];
  __shared__ __attribute__((aligned(16))) float qs[QC * DH];
  __shared__ __attribute__((aligned(16))) float os[QC * DH];
  __shared__ __attribute__((aligned(16))) float dss[QC * (NL + 4)];
  __shared__ float lse_s[QC], dd_s[QC];
  const int tid = threadIdx.x, blk = blockIdx.x, bh = blockIdx.y, nh = a.nh;
  const int key0 = MODE == GB_A3 ? blk * NL : 0;
  const int q_begin = MODE == GB_A1 ? blk * NL : 0;
  const float* Q = a.q + (bh / nh) * a.q_bag + (bh % nh) * a.q_head;
  const float* dO = a.dO + (bh / nh) * a.o_bag + (bh % nh) * a.o_head;
  const float* K = a.k + bh * a.kv_bh + (size_t)key0 * DH;
  const float* V = a.v + bh * a.kv_bh + (size_t)key0 * DH;
  const float* lse = a.lse + bh * a.lq_bh;
  float kreg[DH], vreg[DH], dkacc[DH], dvacc[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const f32x4 t = *(const f32x4*)(K + (size_t)tid * DH + d), u = *(const f32x4*)(V + (size_t)tid * DH + d);
    *(f32x4*)(ks + tid * DH + d) = t;
#pragma unroll
    for (int e = 0; e < 4; ++e) { kreg[d + e] = t[e]; vreg[d + e] = u[e]; dkacc[d + e] = 0.f; dvacc[d + e] = 0.f; }
  }
  const int qi = tid / P4, d4 = (tid % P4) * 4;
#pragma unroll 1
  for (int c0 = 0; c0 < NL; c0 += QC) {
    const int qa = q_begin + c0;
    __syncthreads();   // previous chunk consumed
    *(f32x4*)(qs + qi * DH + d4) = *(const f32x4*)(Q + (size_t)(qa + qi) * a.q_row + d4);
    *(f32x4*)(os + qi * DH + d4) = *(const f32x4*)(dO + (size_t)(qa + qi) * a.o_row + d4);
    if (tid < QC) {
      lse_s[tid] = lse[qa + tid];
      if (MODE == GB_A3) {
        const float* orow = a.o + ((size_t)bh * NL + qa + tid) * DH;
        const float* grow = dO + (size_t)(qa + tid) * a.o_row;
        float dd = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
          const f32x4 g = *(const f32x4*)(grow + d), o = *(const f32x4*)(orow + d);
          dd = fmaf(g[0], o[0], dd); dd = fmaf(g[1], o[1], dd); dd = fmaf(g[2], o[2], dd); dd = fmaf(g[3], o[3], dd);
        }
        dd_s[tid] = dd;
      } else {
        dd_s[tid] = a.dd[bh * a.lq_bh + qa + tid];
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int qq = 0; qq < QC; ++qq) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; d += 4) {
        const f32x4 q4 = *(const f32x4*)(qs + qq * DH + d), o4 = *(const f32x4*)(os + qq * DH + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) { s = fmaf(q4[e], kreg[d + e], s); dp = fmaf(o4[e], vreg[d + e], dp); }
      }
      const float p = __expf(s - lse_s[qq]);
      const float ds = p * (dp - dd_s[qq]);
      dss[qq * (NL + 4) + tid] = ds;
#pragma unroll
      for (int d = 0; d < DH; d += 4) {
        const f32x4 q4 = *(const f32x4*)(qs + qq * DH + d), o4 = *(const f32x4*)(os + qq * DH + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) { dkacc[d + e] = fmaf(ds, q4[e], dkacc[d + e]); dvacc[d + e] = fmaf(p, o4[e], dvacc[d + e]); }
      }
    }
    __syncthreads();
    f32x4 part[4] = {};   // four interleaved partial sums, combined pairwise
#pragma unroll 4
    for (int key = 0; key < NL; key += 4) {
      const f32x4 s4 = *(const f32x4*)(dss + qi * (NL + 4) + key);
#pragma unroll
      for (int i = 0; i < 4; ++i) fma4(part[i], s4[i], *(const f32x4*)(ks + (key + i) * DH + d4));
    }
    const f32x4 acc = (part[0] + part[1]) + (part[2] + part[3]);
    float* dqd = a.dq + bh * a.dq_bh + (MODE == GB_A3 ? blk * a.dq_slab : 0);
    *(f32x4*)(dqd + (size_t)(qa + qi) * DH + d4) = acc;
  }
  float* dkd;
  float* dvd;
  if (MODE == GB_A3) {
    dkd = a.dk + bh * a.dkv_bh + (size_t)key0 * DH;
    dvd = a.dv + bh * a.dkv_bh + (size_t)key0 * DH;
  } else {
    dkd = a.dk + blk * a.dkv_slab + bh * a.dkv_bh;
    dvd = a.dv + blk * a.dkv_slab + bh * a.dkv_bh;
  }
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    f32x4 gk = {dkacc[d], dkacc[d + 1], dkacc[d + 2], dkacc[d + 3]};
    f32x4 gv = {dvacc[d], dvacc[d + 1], dvacc[d + 2], dvacc[d + 3]};
    if (MODE == GB_A3) gv += *(const f32x4*)(dvd + (size_t)tid * DH + d);
    *(f32x4*)(dkd + (size_t)tid * DH + d) = gk;
    *(f32x4*)(dvd + (size_t)tid * DH + d) = gv;
  }
}

// ---------------------------------------------------------------------------
// dqkv[bag][t][which*h*DH + head*DH + d]:
//   q: scale * (dq[t] + dql[t/l] / l);  k: dk[t] + dkl[t/l] / l;  v: dv[t]
// item = (t, 8 consecutive columns); grid (ceil(n * 3*nh*DH/8 / 256), nbags), block 256
template <typename T, int DH, int NL>
__global__ __launch_bounds__(256) void assemble_dqkv_g(const float* __restrict__ dq, const float* __restrict__ dql,
                                                       const float* __restrict__ dk, const float* __restrict__ dkl,
                                                       const float* __restrict__ dv, int n, int l, int nh, float scale,
                                                       T* __restrict__ dqkv) {
  const int inner = nh * DH, per_row = 3 * inner / 8;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)n * per_row) return;
  const int c = (int)(item % per_row) * 8;
  const int t = (int)(item / per_row), bag = blockIdx.y;
  const int which = c / inner, head = (c % inner) / DH, d = c % DH;   // DH % 8 == 0: never straddles a head
  const size_t bh = (size_t)bag * nh + head;
  const size_t row = (bh * n + t) * DH + d;
  const size_t lrow = (bh * NL + t / l) * DH + d;
  const float inv_l = 1.0f / (float)l;
  const float* src = which == 0 ? dq : which == 1 ? dk : dv;
  const float* lsrc = which == 0 ? dql : dkl;
  const f32x8 a = load8<float>(src + row);
  f32x8 b = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (which < 2) b = load8<float>(lsrc + lrow);
  vec8<T> out;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float val;
    if (which == 0) val = scale * (a[e] + b[e] * inv_l);
    else if (which == 1) val = a[e] + b[e] * inv_l;
    else val = a[e];
    out[e] = from_f<T>(val);
  }
  store8<T>(dqkv + ((size_t)bag * n + t) * (3 * inner) + c, out);
}

// ---------------------------------------------------------------------------
// Row `row` of attn1 Z attn3 (attn_rows.hip for this family): grid (n / NL, nbh), block NL, one
// token per thread;  out[t] = sum_j w_j exp(ql_j . k_t - lse3_j),  w = softmax(q_r kl^T) Z
template <int DH, int NL>
__global__ __launch_bounds__(NL) void attn_row_g(const float* __restrict__ q, const float* __restrict__ k,
                                                 const float* __restrict__ ql, const float* __restrict__ kl,
                                                 const float* __restrict__ z, const float* __restrict__ lse3, int n,
                                                 int row, float* __restrict__ out) {
  constexpr int NW = NL / 64;
  __shared__ __attribute__((aligned(16))) float qls[NL * DH];
  __shared__ float a1[NL], w[NL], lse[NL], red[2 * NW];
  const int tid = threadIdx.x, bh = blockIdx.y;
  const size_t hq = (size_t)bh * n * DH, hl = (size_t)bh * NL * DH;
  float s = 0.f;
  {
    const float* qr = q + hq + (size_t)row * DH;
    const float* kj = kl + hl + (size_t)tid * DH;
#pragma unroll 8
    for (int d = 0; d < DH; ++d) s = fmaf(qr[d], kj[d], s);
  }
  float m = wave_max(s);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) m = fmaxf(m, red[i]);
  const float e = expf(s - m);
  float sum = wave_sum(e);
  if ((tid & 63) == 0) red[NW + (tid >> 6)] = sum;
  __syncthreads();
  sum = red[NW];
#pragma unroll
  for (int i = 1; i < NW; ++i) sum += red[NW + i];
  a1[tid] = e / sum;
  lse[tid] = lse3[(size_t)bh * NL + tid];
  for (int c = tid; c < NL * DH / 4; c += NL) *(f32x4*)(qls + c * 4) = *(const f32x4*)(ql + hl + (size_t)c * 4);
  __syncthreads();
  {
    const float* zh = z + (size_t)bh * NL * NL;
    float acc = 0.f;
#pragma unroll 8
    for (int j = 0; j < NL; ++j) acc = fmaf(a1[j], zh[(size_t)j * NL + tid], acc);
    w[tid] = acc;
  }
  __syncthreads();
  const int t = blockIdx.x * NL + tid;   // n is a multiple of NL: t < n
  float kr[DH];
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const f32x4 x = *(const f32x4*)(k + hq + (size_t)t * DH + d);
    kr[d] = x[0]; kr[d + 1] = x[1]; kr[d + 2] = x[2]; kr[d + 3] = x[3];
  }
  float acc = 0.f;
  for (int j = 0; j < NL; ++j) {
    const float* qj = qls + j * DH;   // every lane reads the same row: LDS broadcast
    float d0 = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const f32x4 x = *(const f32x4*)(qj + d);
      d0 = fmaf(x[0], kr[d], d0); d0 = fmaf(x[1], kr[d + 1], d0);
      d0 = fmaf(x[2], kr[d + 2], d0); d0 = fmaf(x[3], kr[d + 3], d0);
    }
    acc = fmaf(w[j], expf(d0 - lse[j]), acc);
  }
  out[(size_t)bh * n + t] = acc;
}

// ---------------------------------------------------------------------------
// Moore-Penrose chain, the kernels around its tm_bmm products (pinv.hip at NL landmarks).
// rowsum / colsum of |X|: grid (nbh, 2), block NL
template <int NL>
__global__ __launch_bounds__(NL) void abs_sums_g(const float* __restrict__ X, float* __restrict__ sums, int nbh) {
  const int bh = blockIdx.x, t = threadIdx.x;
  const float* x = X + (size_t)bh * NL * NL;
  float s = 0.f;
  if (blockIdx.y == 0) {
    for (int j = 0; j < NL; ++j) s += fabsf(x[(size_t)t * NL + j]);
    sums[(size_t)bh * NL + t] = s;
  } else {
    for (int i = 0; i < NL; ++i) s += fabsf(x[(size_t)i * NL + t]);
    sums[(size_t)(nbh + bh) * NL + t] = s;
  }
}

struct MaxInfoG { float maxc, maxr, nc, nr; };

// the maxima over ALL bags and heads (and how many entries tie with each); red: 2 * NL / 64 floats
template <int NL>
TM_DEV MaxInfoG block_maxima_g(const float* sums, int nbh, float* red) {
  constexpr int NW = NL / 64;
  const int t = threadIdx.x, total = nbh * NL;
  float mc = -INFINITY, mr = -INFINITY;
  for (int i = t; i < total; i += NL) { mc = fmaxf(mc, sums[i]); mr = fmaxf(mr, sums[total + i]); }
  mc = wave_max(mc); mr = wave_max(mr);
  if ((t & 63) == 0) { red[t >> 6] = mc; red[NW + (t >> 6)] = mr; }
  __syncthreads();
  MaxInfoG mi;
  mi.maxc = red[0]; mi.maxr = red[NW];
#pragma unroll
  for (int i = 1; i < NW; ++i) { mi.maxc = fmaxf(mi.maxc, red[i]); mi.maxr = fmaxf(mi.maxr, red[NW + i]); }
  __syncthreads();
  float nc = 0.f, nr = 0.f;
  for (int i = t; i < total; i += NL) { nc += sums[i] == mi.maxc; nr += sums[total + i] == mi.maxr; }
  nc = wave_sum(nc); nr = wave_sum(nr);
  if ((t & 63) == 0) { red[t >> 6] = nc; red[NW + (t >> 6)] = nr; }
  __syncthreads();
  mi.nc = red[0]; mi.nr = red[NW];
#pragma unroll
  for (int i = 1; i < NW; ++i) { mi.nc += red[i]; mi.nr += red[NW + i]; }
  __syncthreads();
  return mi;
}

// Z0[bh][i][j] = X[bh][j][i] / (maxc * maxr); grid (nbh, NL / 16), block NL (16 rows of Z0 each)
template <int NL>
__global__ __launch_bounds__(NL) void pinv_init_g(const float* __restrict__ X, const float* __restrict__ sums, int nbh,
                                                  float* __restrict__ Z0, float* __restrict__ stats) {
  __shared__ float red[2 * NL / 64];
  __shared__ float tile[NL][17];
  const MaxInfoG mi = block_maxima_g<NL>(sums, nbh, red);
  const float denom = mi.maxc * mi.maxr;
  const int bh = blockIdx.x, i0 = blockIdx.y * 16, t = threadIdx.x;
  const float* x = X + (size_t)bh * NL * NL;
  for (int e = t; e < NL * 16; e += NL) {
    const int j = e >> 4, ii = e & 15;
    tile[j][ii] = x[(size_t)j * NL + i0 + ii];
  }
  __syncthreads();
  for (int ii = 0; ii < 16; ++ii) Z0[((size_t)bh * NL + i0 + ii) * NL + t] = tile[t][ii] / denom;
  if (bh == 0 && blockIdx.y == 0 && t == 0) {
    stats[0] = mi.maxc; stats[1] = mi.maxr; stats[2] = denom; stats[3] = mi.nc; stats[4] = mi.nr;
  }
}

// partial sums of G0 * Z0 over 16-row slices: grid (nbh, NL / 16), block 256
template <int NL>
__global__ __launch_bounds__(256) void dot_partial_g(const float* __restrict__ G, const float* __restrict__ Z,
                                                     float* __restrict__ part) {
  __shared__ float red[4];
  const size_t base = ((size_t)blockIdx.x * NL + blockIdx.y * 16) * NL;
  float s = 0.f;
  for (int e = threadIdx.x; e < 16 * NL; e += 256) s += G[base + e] * Z[base + e];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x * gridDim.y + blockIdx.y] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dX[bh][i][j] += G0[bh][j][i]/denom + sign(X_ij) * (tie_c(bh,i) dMc/nc + tie_r(bh,j) dMr/nr)
// with dc = -sum(G0*Z0)/denom, dMc = dc*maxr, dMr = dc*maxc.  grid (nbh, NL / 16), block NL
template <int NL>
__global__ __launch_bounds__(NL) void pinv_init_bwd_g(const float* __restrict__ X, const float* __restrict__ sums,
                                                      const float* __restrict__ G0, const float* __restrict__ gz,
                                                      int nbh, float* __restrict__ dX) {
  __shared__ float red[2 * NL / 64];
  __shared__ float tile[NL][17];
  const MaxInfoG mi = block_maxima_g<NL>(sums, nbh, red);
  const float denom = mi.maxc * mi.maxr;
  const float dc = -gz[0] / denom;
  const float dMc = dc * mi.maxr / mi.nc, dMr = dc * mi.maxc / mi.nr;
  const int bh = blockIdx.x, i0 = blockIdx.y * 16, t = threadIdx.x;
  const float* g = G0 + (size_t)bh * NL * NL;
  for (int e = t; e < NL * 16; e += NL) {
    const int j = e >> 4, ii = e & 15;
    tile[j][ii] = g[(size_t)j * NL + i0 + ii];
  }
  __syncthreads();
  const float* rs = sums + (size_t)bh * NL;
  const float* cs = sums + (size_t)(nbh + bh) * NL;
  const float tie_r = cs[t] == mi.maxr ? dMr : 0.f;
  for (int ii = 0; ii < 16; ++ii) {
    const int i = i0 + ii;
    const size_t off = ((size_t)bh * NL + i) * NL + t;
    const float xv = X[off];
    const float sg = xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f);
    const float tie_c = rs[i] == mi.maxc ? dMc : 0.f;
    dX[off] += tile[t][ii] / denom + sg * (tie_c + tie_r);
  }
}

tm_bmm_job sq_job(const float* A, int ta, const float* B, int tb, float* C, int m, float alpha, float diag = 0.f) {
  tm_bmm_job j{};
  j.A = A; j.ta = ta; j.B = B; j.tb = tb;
  j.lda = m; j.ldb = m;
  j.sa = (long long)m * m; j.sb = (long long)m * m;
  j.C = C; j.ldc = m; j.sc = (long long)m * m;
  j.M = m; j.N = m; j.K = m;
  j.alpha = alpha; j.diag = diag;
  return j;
}
void sq_add_term(tm_bmm_job& j, const float* A, int ta, const float* B, int tb) {
  j.A2 = A; j.ta2 = ta; j.B2 = B; j.tb2 = tb;
  j.lda2 = j.M; j.ldb2 = j.M;
  j.sa2 = (long long)j.M * j.M; j.sb2 = (long long)j.M * j.M;
}

}  // namespace

// ============================ C entry points ===============================
#define TM_NYSG_SHAPE(name, dh, nl, nbh, n)                                              \
  TM_GEO_REQUIRE(dh, nl);                                                                \
  TM_REQUIRE((n) > 0 && (n) % (nl) == 0, name ": n must be a positive multiple of nl");  \
  TM_REQUIRE((nbh) > 0, name ": nbh must be positive")

extern "C" int tm_nysg_landmarks(int dh, int nl, const float* q, const float* k, int nbh, int n, float* ql, float* kl,
                                 void* stream) {
  TM_NYSG_SHAPE("nysg_landmarks", dh, nl, nbh, n);
  TM_REQUIRE(q && k && ql && kl, "nysg_landmarks: null pointer");
  const long long rows = (long long)nbh * nl, items = rows * (dh / 4);
  const dim3 grid((unsigned)((items + 255) / 256), 2);
  TM_GEO_DISPATCH(dh, ((void)NL, landmarks_g<DH><<<grid, 256, 0, (hipStream_t)stream>>>(q, k, rows, n / nl, ql, kl)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_nysg_a3_workspace(int dh, int nl, int nbh, int n) {
  if (!geo_ok(dh, nl) || nbh <= 0 || n <= 0 || n % nl) return -1;
  return (long long)(n / nl) * nbh * nl * (dh + 2) * (long long)sizeof(float);
}

extern "C" int tm_nysg_a3_fwd(int dh, int nl, const float* ql, const float* k, const float* v, int nbh, int n,
                              float* work, float* w, float* lse3, void* stream) {
  TM_NYSG_SHAPE("nysg_a3_fwd", dh, nl, nbh, n);
  TM_REQUIRE(ql && k && v && work && w && lse3, "nysg_a3_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int nkb = n / nl;
  float* po = work;
  float* pm = po + (size_t)nkb * nbh * nl * dh;
  float* pl = pm + (size_t)nkb * nbh * nl;
  const long long items = (long long)nbh * nl * (dh / 4);
  TM_GEO_DISPATCH(dh, (a3_fwd_g<DH, NL><<<dim3(nkb, nbh, NL / QPW), NL, 0, st>>>(ql, k, v, n, po, pm, pl)));
  TM_CHECK_LAUNCH();
  TM_GEO_DISPATCH(dh, (a3_combine_g<DH, NL><<<(unsigned)((items + 255) / 256), 256, 0, st>>>(po, pm, pl, nkb, nbh, w,
                                                                                            lse3)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nysg_sim2_softmax(int dh, int nl, const float* ql, const float* kl, int nbh, float* a2,
                                    void* stream) {
  TM_GEO_REQUIRE(dh, nl);
  TM_REQUIRE(nbh > 0, "nysg_sim2_softmax: nbh must be positive");
  TM_REQUIRE(ql && kl && a2, "nysg_sim2_softmax: null pointer");
  tm_bmm_job j{};   // logits = ql kl^T (exact fp32), then the row softmax in place
  j.A = ql; j.ta = 0; j.lda = dh; j.sa = (long long)nl * dh;
  j.B = kl; j.tb = 1; j.ldb = dh; j.sb = (long long)nl * dh;
  j.C = a2; j.ldc = nl; j.sc = (long long)nl * nl;
  j.M = nl; j.N = nl; j.K = dh;
  j.alpha = 1.f;
  if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
  const long long rows = (long long)nbh * nl;
  TM_NL_DISPATCH(nl, (softmax_rows_g<NL><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(a2, rows)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nysg_softmax_bwd_rows(int dh, int nl, const float* a, const float* da, float* ds, long long rows,
                                        void* stream) {
  TM_GEO_REQUIRE(dh, nl);
  TM_REQUIRE(rows > 0, "nysg_softmax_bwd_rows: rows must be positive");
  TM_REQUIRE(a && da && ds, "nysg_softmax_bwd_rows: null pointer");
  TM_NL_DISPATCH(nl, (softmax_bwd_rows_g<NL><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(a, da, ds,
                                                                                                          rows)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nysg_mm(int dh, int nl, const float* A, int ta, const float* B, const float* E1, float e1, float* C,
                          int nbh, void* stream) {
  TM_GEO_REQUIRE(dh, nl);
  TM_REQUIRE(nbh > 0 && (ta == 0 || ta == 1), "nysg_mm: nbh must be positive, ta 0 or 1");
  TM_REQUIRE(A && B && C, "nysg_mm: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (ta) { TM_GEO_DISPATCH(dh, (mm_g<DH, NL, 1><<<dim3(NL / QC, nbh), NL, 0, st>>>(A, B, E1, e1, C))); }
  else { TM_GEO_DISPATCH(dh, (mm_g<DH, NL, 0><<<dim3(NL / QC, nbh), NL, 0, st>>>(A, B, E1, e1, C))); }
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nysg_a1_fwd(int dh, int nl, const float* q, const float* v, const float* kl, const float* y,
                              const float* wconv, int nbh, int nh, int n, float* merged, float* lse1, void* stream) {
  TM_NYSG_SHAPE("nysg_a1_fwd", dh, nl, nbh, n);
  TM_REQUIRE(nh > 0 && nbh % nh == 0, "nysg_a1_fwd: nbh must be a multiple of nh");
  TM_REQUIRE(q && v && kl && y && wconv && merged && lse1, "nysg_a1_fwd: null pointer");
  TM_GEO_DISPATCH(dh, (a1_fwd_g<DH, NL><<<dim3(n / QPW, nbh), NL, 0, (hipStream_t)stream>>>(q, v, kl, y, wconv, n, nh,
                                                                                           merged, lse1)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_nysg_conv_bwd_workspace(int dh, int nl, int nbags, int nh, int n) {
  if (!geo_ok(dh, nl) || nbags <= 0 || nh <= 0 || n <= 0 || n % nl) return -1;
  return (long long)nbags * (n / CB_R) * nh * TAPS * (long long)sizeof(float);
}

extern "C" int tm_nysg_conv_bwd(int dh, int nl, const float* dmerged, const float* merged, const float* v,
                                const float* wconv, int nbh, int nh, int n, float* dv, float* d1, float* work,
                                float* dwconv, tm_reduce_queue* rq, void* stream) {
  TM_NYSG_SHAPE("nysg_conv_bwd", dh, nl, nbh, n);
  TM_REQUIRE(nh > 0 && nbh % nh == 0, "nysg_conv_bwd: nbh must be a multiple of nh");
  TM_REQUIRE(dmerged && merged && v && wconv && dv && d1 && work && dwconv, "nysg_conv_bwd: null pointer");
  const int ntb = n / CB_R;   // nl is a multiple of CB_R
  TM_GEO_DISPATCH(dh, ((void)NL, conv_bwd_g<DH><<<dim3(ntb, nbh), 256, 0, (hipStream_t)stream>>>(
                                     dmerged, merged, v, wconv, n, nh, dv, d1, work)));
  TM_CHECK_LAUNCH();
  return tm_splitk_reduce(work, dwconv, (nbh / nh) * ntb, (long long)nh * TAPS, 1.0f, 0, rq, stream);
}

extern "C" long long tm_nysg_a1_bwd_workspace(int dh, int nl, int nbh, int n) {
  if (!geo_ok(dh, nl) || nbh <= 0 || n <= 0 || n % nl) return -1;
  return 2LL * (n / nl) * nbh * nl * dh * (long long)sizeof(float);
}

extern "C" int tm_nysg_a1_bwd(int dh, int nl, const float* q, const float* dmerged, const float* kl, const float* y,
                              const float* lse1, const float* d1, int nbh, int nh, int n, float* dq, float* work,
                              float* dkl, float* dy, tm_reduce_queue* rq, void* stream) {
  TM_NYSG_SHAPE("nysg_a1_bwd", dh, nl, nbh, n);
  TM_REQUIRE(nh > 0 && nbh % nh == 0, "nysg_a1_bwd: nbh must be a multiple of nh");
  TM_REQUIRE(q && dmerged && kl && y && lse1 && d1 && dq && work && dkl && dy, "nysg_a1_bwd: null pointer");
  const int nqc = n / nl;
  const long long cnt = (long long)nbh * nl * dh;
  GBwdArgs a{};
  a.q = q; a.q_bag = (long long)nh * n * dh; a.q_head = (long long)n * dh; a.q_row = dh;
  a.dO = dmerged; a.o_bag = (long long)n * nh * dh; a.o_head = dh; a.o_row = nh * dh;
  a.k = kl; a.v = y; a.kv_bh = (long long)nl * dh;
  a.lse = lse1; a.dd = d1; a.lq_bh = n;
  a.dq = dq; a.dq_bh = (long long)n * dh;
  a.dk = work; a.dv = work + (size_t)nqc * cnt; a.dkv_bh = (long long)nl * dh; a.dkv_slab = cnt;
  a.nh = nh;
  TM_GEO_DISPATCH(dh, (attn_bwd_g<DH, NL, GB_A1><<<dim3(nqc, nbh), NL, 0, (hipStream_t)stream>>>(a)));
  TM_CHECK_LAUNCH();
  if (int rc = tm_splitk_reduce(a.dk, dkl, nqc, cnt, 1.0f, 0, rq, stream)) return rc;
  return tm_splitk_reduce(a.dv, dy, nqc, cnt, 1.0f, 0, rq, stream);
}

extern "C" long long tm_nysg_a3_bwd_workspace(int dh, int nl, int nbh, int n) {
  if (!geo_ok(dh, nl) || nbh <= 0 || n <= 0 || n % nl) return -1;
  return (long long)(n / nl) * nbh * nl * dh * (long long)sizeof(float);
}

extern "C" int tm_nysg_a3_bwd(int dh, int nl, const float* ql, const float* dw, const float* w, const float* k,
                              const float* v, const float* lse3, int nbh, int n, float* dk, float* dv, float* work,
                              float* dql, tm_reduce_queue* rq, void* stream) {
  TM_NYSG_SHAPE("nysg_a3_bwd", dh, nl, nbh, n);
  TM_REQUIRE(ql && dw && w && k && v && lse3 && dk && dv && work && dql, "nysg_a3_bwd: null pointer");
  const int nkb = n / nl;
  const long long cnt = (long long)nbh * nl * dh;
  GBwdArgs a{};
  a.q = ql; a.q_bag = 0; a.q_head = (long long)nl * dh; a.q_row = dh;   // nh = 1: bh indexes heads directly
  a.dO = dw; a.o_bag = 0; a.o_head = (long long)nl * dh; a.o_row = dh;
  a.k = k; a.v = v; a.kv_bh = (long long)n * dh;
  a.lse = lse3; a.lq_bh = nl; a.o = w;
  a.dq = work; a.dq_bh = (long long)nl * dh; a.dq_slab = cnt;
  a.dk = dk; a.dv = dv; a.dkv_bh = (long long)n * dh;
  a.nh = nbh;   // bh / nh == 0, bh % nh == bh
  TM_GEO_DISPATCH(dh, (attn_bwd_g<DH, NL, GB_A3><<<dim3(nkb, nbh), NL, 0, (hipStream_t)stream>>>(a)));
  TM_CHECK_LAUNCH();
  return tm_splitk_reduce(work, dql, nkb, cnt, 1.0f, 0, rq, stream);
}

extern "C" int tm_nysg_assemble_dqkv(int dh, int nl, int dtype, const float* dq, const float* dql, const float* dk,
                                     const float* dkl, const float* dv, int nbags, int nh, int n, float scale,
                                     void* dqkv, void* stream) {
  TM_NYSG_SHAPE("nysg_assemble_dqkv", dh, nl, nbags, n);
  TM_REQUIRE(dtype == TM_F32 || dtype == TM_BF16, "nysg_assemble_dqkv: dtype must be TM_F32 or TM_BF16");
  TM_REQUIRE(nh > 0 && dq && dql && dk && dkl && dv && dqkv, "nysg_assemble_dqkv: null pointer");
  const long long items = (long long)n * 3 * nh * dh / 8;
  const dim3 grid((unsigned)((items + 255) / 256), nbags);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) {
    TM_GEO_DISPATCH(dh, (assemble_dqkv_g<bf16, DH, NL><<<grid, 256, 0, st>>>(dq, dql, dk, dkl, dv, n, n / NL, nh, scale,
                                                                            (bf16*)dqkv)));
  } else {
    TM_GEO_DISPATCH(dh, (assemble_dqkv_g<float, DH, NL><<<grid, 256, 0, st>>>(dq, dql, dk, dkl, dv, n, n / NL, nh, scale,
                                                                             (float*)dqkv)));
  }
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nysg_attn_row(int dh, int nl, const float* q, const float* k, const float* ql, const float* kl,
                                const float* z, const float* lse3, int nbh, int n, int row, float* out, void* stream) {
  TM_NYSG_SHAPE("nysg_attn_row", dh, nl, nbh, n);
  TM_REQUIRE(q && k && ql && kl && z && lse3 && out, "nysg_attn_row: null pointer");
  TM_REQUIRE(row >= 0 && row < n, "nysg_attn_row: row out of range");
  TM_GEO_DISPATCH(dh, (attn_row_g<DH, NL><<<dim3(n / NL, nbh), NL, 0, (hipStream_t)stream>>>(q, k, ql, kl, z, lse3, n,
                                                                                            row, out)));
  TM_CHECK_LAUNCH();
  return 0;
}

// saved: Zs[iters+1], Ps[iters], T3s[iters], T5s[iters] (each nbh*nl*nl fp32) + sums[2][nbh][nl] + stats[8]
extern "C" long long tm_nysg_pinv_saved_floats(int dh, int nl, int nbh, int iters) {
  if (!geo_ok(dh, nl) || nbh <= 0 || iters < 1) return -1;
  return (4LL * iters + 1) * nbh * nl * nl + 2LL * nbh * nl + 8;
}

extern "C" int tm_nysg_pinv_fwd(int dh, int nl, const float* X, int nbh, int iters, float* saved, void* stream) {
  TM_GEO_REQUIRE(dh, nl);
  TM_REQUIRE(nbh > 0 && iters >= 1, "nysg_pinv_fwd: nbh and iters must be positive");
  TM_REQUIRE(X && saved, "nysg_pinv_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int m = nl;
  const size_t mat = (size_t)nbh * m * m;
  float* Zs = saved;
  float* Ps = Zs + (iters + 1) * mat;
  float* T3s = Ps + iters * mat;
  float* T5s = T3s + iters * mat;
  float* sums = T5s + iters * mat;
  float* stats = sums + 2 * (size_t)nbh * m;
  TM_NL_DISPATCH(nl, (abs_sums_g<NL><<<dim3(nbh, 2), NL, 0, st>>>(X, sums, nbh)));
  TM_CHECK_LAUNCH();
  TM_NL_DISPATCH(nl, (pinv_init_g<NL><<<dim3(nbh, NL / 16), NL, 0, st>>>(X, sums, nbh, Zs, stats)));
  TM_CHECK_LAUNCH();
  {
    tm_bmm_job j = sq_job(X, 0, Zs, 0, Ps, m, 1.f);                       // P_0 = X Z_0
    if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
  }
  // Each iteration computes P_k = X Z_k from the current Z (pinv.hip's 512-wide schedule advances
  // P by its own recurrence, 2 dependent launches per iteration instead of 4; the direct product
  // keeps the iteration self-correcting: a rounding error in Z_k is seen by P_k and damped)
  for (int it = 0; it < iters; ++it) {
    float* P = Ps + it * mat;
    float* T3 = T3s + it * mat;
    float* T5 = T5s + it * mat;
    float* Z = Zs + it * mat;
    float* Zn = Zs + (it + 1) * mat;   // also the scratch of R = P P until Z_{it+1} is written
    tm_bmm_job j = sq_job(P, 0, P, 0, Zn, m, 1.f);                        // R = P P
    j.E1 = P;
    j.C2 = T3; j.c2_alpha = 1.f; j.c2_diag = 15.f; j.c2_e1 = -7.f;        // T3 = R - 7P + 15I
    if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
    j = sq_job(P, 0, T3, 0, T5, m, -1.f, 13.f);                           // T5 = 13I - P T3
    if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
    j = sq_job(Z, 0, T5, 0, Zn, m, 0.25f);                                // Z_{it+1} = 0.25 Z T5
    if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
    if (it + 1 < iters) {
      j = sq_job(X, 0, Zn, 0, Ps + (it + 1) * mat, m, 1.f);               // P_{it+1} = X Z_{it+1}
      if (int rc = tm_bmm(&j, 1, nbh, 0, stream)) return rc;
    }
  }
  return 0;
}

// workspace: 5 matrices + partial dots (nbh * 16) + 16
extern "C" long long tm_nysg_pinv_bwd_workspace_floats(int dh, int nl, int nbh) {
  if (!geo_ok(dh, nl) || nbh <= 0) return -1;
  return 5LL * nbh * nl * nl + nbh * 16LL + 16;
}

// dZ (gradient w.r.t. the final Z) is consumed (overwritten).  dX is written (=).
extern "C" int tm_nysg_pinv_bwd(int dh, int nl, const float* X, int nbh, int iters, const float* saved, float* dZ,
                                float* work, float* dX, void* stream) {
  TM_GEO_REQUIRE(dh, nl);
  TM_REQUIRE(nbh > 0 && iters >= 1, "nysg_pinv_bwd: nbh and iters must be positive");
  TM_REQUIRE(X && saved && dZ && work && dX, "nysg_pinv_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int m = nl;
  const size_t mat = (size_t)nbh * m * m;
  const float* Zs = saved;
  const float* Ps = Zs + (iters + 1) * mat;
  const float* T3s = Ps + iters * mat;
  const float* T5s = T3s + iters * mat;
  const float* sums = T5s + iters * mat;
  float* dT5 = work;
  float* dZa = dT5 + mat;
  float* dP = dZa + mat;
  float* dT3 = dP + mat;
  float* part = dT3 + 2 * mat;
  float* gz = part + nbh * 16;
  float* G = dZ;
  bool first = true;
  for (int it = iters - 1; it >= 0; --it) {
    const float* Z = Zs + it * mat;
    const float* P = Ps + it * mat;
    const float* T3 = T3s + it * mat;
    const float* T5 = T5s + it * mat;
    tm_bmm_job jb[2];
    jb[0] = sq_job(Z, 1, G, 0, dT5, m, 0.25f);                            // dT5 = 0.25 Z^T G
    jb[1] = sq_job(G, 0, T5, 1, dZa, m, 0.25f);                           // dZa = 0.25 G T5^T
    if (int rc = tm_bmm(jb, 2, nbh, 0, stream)) return rc;
    jb[0] = sq_job(dT5, 0, T3, 1, dP, m, -1.f);                           // dP  = -dT5 T3^T
    jb[1] = sq_job(P, 1, dT5, 0, dT3, m, -1.f);                           // dT3 = -P^T dT5
    if (int rc = tm_bmm(jb, 2, nbh, 0, stream)) return rc;
    jb[0] = sq_job(dT3, 0, P, 1, dP, m, 1.f);                             // dP += dT3 P^T + P^T dT3 - 7 dT3
    sq_add_term(jb[0], P, 1, dT3, 0);
    jb[0].E1 = dP; jb[0].e1 = 1.f; jb[0].E2 = dT3; jb[0].e2 = -7.f;
    if (int rc = tm_bmm(jb, 1, nbh, 0, stream)) return rc;
    jb[0] = sq_job(dP, 0, Z, 1, dX, m, 1.f);                              // dX (+)= dP Z^T
    if (!first) { jb[0].E1 = dX; jb[0].e1 = 1.f; }
    jb[1] = sq_job(X, 1, dP, 0, G, m, 1.f);                               // G = dZa + X^T dP
    jb[1].E1 = dZa; jb[1].e1 = 1.f;
    if (int rc = tm_bmm(jb, 2, nbh, 0, stream)) return rc;
    first = false;
  }
  // init: Z0 = X^T / (maxc * maxr)
  TM_NL_DISPATCH(nl, (dot_partial_g<NL><<<dim3(nbh, NL / 16), 256, 0, st>>>(G, Zs, part)));
  TM_CHECK_LAUNCH();
  if (int rc = tm_splitk_reduce(part, gz, nbh * (nl / 16), 1, 1.0f, 0, nullptr, stream)) return rc;   // read below
  TM_NL_DISPATCH(nl, (pinv_init_bwd_g<NL><<<dim3(nbh, NL / 16), NL, 0, st>>>(X, sums, G, gz, nbh, dX)));
  TM_CHECK_LAUNCH();
  return 0;
}
