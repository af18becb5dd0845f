// DTFD-MIL (code/models/model_interface_dtfd.py:174-279 on the blocks of code/models/DTFDMIL.py):
// double-tier gated attention pooling over G pseudo-bags of S instances, fp32, the non-GEMM part.
//   tier 1, pseudo-bag g (rows g S .. g S + S - 1 of the gathered h and Z = h [Wv;Wu]^T + [bv;bu]):
//     a_i   = w . (tanh(Z[i, :D]) * sigmoid(Z[i, D:])) + b          Attention_Gated, K = 1 (:14-45)
//     p     = softmax_S(a) ;  M_g = sum_i p_i h_i ;  sub_g = Wc M_g + bc   (forward :189-209)
//     cam[g, i, c] = p_i (h_i . Wc[c])                               get_cam_1d (:204-205, 691-694)
//   tier 2 (Attention_with_Classifier, DTFDMIL.py:47-56) over the G rows of M:
//     a2_g  = w2 . (tanh(Wv2 M_g + bv2) * sigmoid(Wu2 M_g + bu2)) + b2 ;  p2 = softmax_G(a2)
//     F = sum_g p2_g M_g ;  slide = Wc2 F + bc2 ;  Y_prob = softmax(slide) ;  Y_hat = argmax (:217-220)
//   losses (:236-241, label y on the device): sub_loss = mean_g CE(sub_g, y), slide_loss = CE(slide, y)
// Forward, two stream-ordered launches:
//   t1_fwd_kernel  one workgroup per pseudo-bag: a wave per row computes the score from one read of
//                  the Z row; the block takes the maximum, exp(a - m) and the sum (no exp of an
//                  unshifted score); eight row slices add p_i h_i from one read of each h row and are
//                  then added in slice order; a wave per class writes sub_g.  cam, when asked for, is a
//                  second read of the h rows.
//   t2_fwd_kernel  one workgroup: the G x 2D gate products on 16-row chunks of M staged in LDS (a wave
//                  per gate column, its two weight rows in registers), the softmax over G, F, slide,
//                  both cross entropies, Y_prob and Y_hat.
// Backward, three launches (the first alone when only attCls needs gradients):
//   t2_bwd_kernel  ceil(D / 8) workgroups.  Each recomputes the closed form of tier 2 (d slide, dF,
//                  da2_g = p2_g ((M_g - F) . dF)) and takes eight gate columns: their
//                  dZ2 over all g, the rows of dWv2 / dWu2 / dbv2 / dbu2 / dw2 (a wave per weight row,
//                  g in order) and its slice's share of dM_g = sum_d' dZ2[g, d'] [Wv2;Wu2][d'].
//                  Workgroup 0 also writes dWc2, dbc2, db2, d sub (with the loss's share), dWc, dbc, dF.
//   t1_bwd_kernel  one workgroup per pseudo-bag: dM_g = p2_g dF + the slices' shares in slice order
//                  + Wc^T dsub_g; a wave per row: da_i = p_i ((h_i - M_g) . dM_g), dZ
//                  through tanh / sigmoid, dh_i = p_i dM_g; the sixteen waves' dw / db partials are
//                  added in wave order.
//   t1_reduce_kernel  dw, db = the pseudo-bags' partials added in order.
// No float atomics: every sum is a fixed tree or an index-ordered loop, so results repeat bitwise.
#include "common.h"
#include "mil_common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int CL = 512;           // L: width of h (m_dim)
constexpr int CMAX = 8;           // classes
constexpr int DMAX = 512;         // D: gate width
constexpr int SMAX = 1024;        // instances per pseudo-bag
constexpr int GMAX = 64;          // pseudo-bags
constexpr int NT = 1024;          // threads per workgroup
constexpr int NW = NT / 64;
constexpr int SLICES = NT / (CL / 4);   // 8 groups of 128 f32x4 columns
constexpr int MCHUNK = 16;        // rows of M staged per step of the tier-2 gate products
constexpr int T2_D = NW / 2;      // gate columns per tier-2 backward workgroup: one weight row per wave

__global__ void __launch_bounds__(NT) t1_fwd_kernel(const float* __restrict__ Z, const float* __restrict__ H, int S,
                                                    int D, int C, const float* __restrict__ w,
                                                    const float* __restrict__ b, const float* __restrict__ Wc,
                                                    const float* __restrict__ bc, float* __restrict__ p1,
                                                    float* __restrict__ M, float* __restrict__ sub,
                                                    float* __restrict__ cam) {
  __shared__ __attribute__((aligned(16))) float ws[DMAX];
  __shared__ __attribute__((aligned(16))) float sc[SMAX];
  __shared__ __attribute__((aligned(16))) float acc_s[SLICES * CL];
  __shared__ __attribute__((aligned(16))) float Ms[CL];
  __shared__ float red[NW];
  const int g = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const float* Zg = Z + (size_t)g * S * 2 * D;
  const float* Hg = H + (size_t)g * S * CL;
  for (int d = t; d < D; d += NT) ws[d] = w[d];
  __syncthreads();
  const float b0 = b[0];
#pragma unroll 1
  for (int j = wv; j < S; j += NW) {
    const float* z = Zg + (size_t)j * 2 * D;
    float acc = 0.f;
    for (int d = 4 * lane; d < D; d += 256) {
      const f32x4 za = *(const f32x4*)(z + d), zb = *(const f32x4*)(z + D + d);
      acc = dot4(gate(za, zb), *(const f32x4*)(ws + d), acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) sc[j] = acc + b0;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = t; j < S; j += NT) m = fmaxf(m, sc[j]);
  m = block_reduce<true, NW>(m, red);
  float s = 0.f;
  for (int j = t; j < S; j += NT) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    s += e;
  }
  s = block_reduce<false, NW>(s, red);
  const float inv = 1.f / s;
  for (int j = t; j < S; j += NT) {
    const float p = sc[j] * inv;
    sc[j] = p;
    p1[(size_t)g * S + j] = p;
  }
  __syncthreads();
  // M_g: slice q adds the rows q, q + 8, ... in order; the eight slices are then added in order
  const int slice = t >> 7, col = (t & 127) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int j = slice; j < S; j += SLICES) acc += sc[j] * *(const f32x4*)(Hg + (size_t)j * CL + col);
  *(f32x4*)(acc_s + slice * CL + col) = acc;
  __syncthreads();
  if (t < CL) {
    float v = acc_s[t];
#pragma unroll
    for (int q = 1; q < SLICES; ++q) v += acc_s[q * CL + t];
    Ms[t] = v;
    M[(size_t)g * CL + t] = v;
  }
  __syncthreads();
  if (wv < C) {
    const float* wc = Wc + (size_t)wv * CL;
    float a = dot4(*(const f32x4*)(Ms + 4 * lane), *(const f32x4*)(wc + 4 * lane), 0.f);
    a = dot4(*(const f32x4*)(Ms + 256 + 4 * lane), *(const f32x4*)(wc + 256 + 4 * lane), a);
    a = wave_sum(a);
    if (lane == 0) sub[(size_t)g * C + wv] = a + bc[wv];
  }
  if (cam == nullptr) return;
#pragma unroll 1
  for (int j = wv; j < S; j += NW) {
    const float* h = Hg + (size_t)j * CL;
    const f32x4 h0 = *(const f32x4*)(h + 4 * lane), h1 = *(const f32x4*)(h + 256 + 4 * lane);
    const float p = sc[j];
    for (int c = 0; c < C; ++c) {
      const float* wc = Wc + (size_t)c * CL;
      float a = dot4(h1, *(const f32x4*)(wc + 256 + 4 * lane), dot4(h0, *(const f32x4*)(wc + 4 * lane), 0.f));
      a = wave_sum(a);
      if (lane == 0) cam[((size_t)g * S + j) * C + c] = p * a;
    }
  }
}

__global__ void __launch_bounds__(NT) t2_fwd_kernel(
    const float* __restrict__ M, int G, int D, int C, const float* __restrict__ Wv2, const float* __restrict__ bv2,
    const float* __restrict__ Wu2, const float* __restrict__ bu2, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ Wc2, const float* __restrict__ bc2,
    const float* __restrict__ sub, const long long* __restrict__ label, float* __restrict__ Z2,
    float* __restrict__ p2, float* __restrict__ Fo, float* __restrict__ slide, float* __restrict__ losses,
    float* __restrict__ yprob, long long* __restrict__ yhat) {
  __shared__ __attribute__((aligned(16))) float Ms[MCHUNK * CL];
  __shared__ float apart[NW * GMAX];
  __shared__ float a2[GMAX];
  __shared__ __attribute__((aligned(16))) float Fs[CL];
  __shared__ float rowloss[GMAX];
  __shared__ float sl[CMAX];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  float acc_g = 0.f;                 // lane g of wave wv: this wave's share of a2[g]
  for (int g0 = 0; g0 < G; g0 += MCHUNK) {
    const int ng = min(MCHUNK, G - g0);
    __syncthreads();
    for (int e = t; e < ng * (CL / 4); e += NT) ((f32x4*)Ms)[e] = ((const f32x4*)(M + (size_t)g0 * CL))[e];
    __syncthreads();
#pragma unroll 1
    for (int d = wv; d < D; d += NW) {
      const float* rv = Wv2 + (size_t)d * CL;
      const float* ru = Wu2 + (size_t)d * CL;
      const f32x4 v0 = *(const f32x4*)(rv + 4 * lane), v1 = *(const f32x4*)(rv + 256 + 4 * lane);
      const f32x4 u0 = *(const f32x4*)(ru + 4 * lane), u1 = *(const f32x4*)(ru + 256 + 4 * lane);
      const float bvd = bv2[d], bud = bu2[d], wd = w2[d];
      for (int gg = 0; gg < ng; ++gg) {
        const f32x4 m0 = *(const f32x4*)(Ms + gg * CL + 4 * lane), m1 = *(const f32x4*)(Ms + gg * CL + 256 + 4 * lane);
        const float zv = wave_sum_dpp(dot4(m1, v1, dot4(m0, v0, 0.f))) + bvd;
        const float zu = wave_sum_dpp(dot4(m1, u1, dot4(m0, u0, 0.f))) + bud;
        if (lane == 0) {
          Z2[(size_t)(g0 + gg) * 2 * D + d] = zv;
          Z2[(size_t)(g0 + gg) * 2 * D + D + d] = zu;
        }
        const float gt = gate(zv, zu);
        if (lane == g0 + gg) acc_g = fmaf(gt, wd, acc_g);
      }
    }
  }
  apart[wv * GMAX + lane] = acc_g;
  __syncthreads();
  if (t < G) {
    float a = b2[0];
#pragma unroll
    for (int q = 0; q < NW; ++q) a += apart[q * GMAX + t];
    a2[t] = a;
  }
  __syncthreads();
  if (wv == 0) {
    const float v = lane < G ? a2[lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < G ? expf(v - m) : 0.f;
    const float s = wave_sum(e);
    if (lane < G) {
      a2[lane] = e / s;
      p2[lane] = e / s;
    }
  }
  __syncthreads();
  if (t < CL) {
    float f = 0.f;
    for (int g = 0; g < G; ++g) f = fmaf(a2[g], M[(size_t)g * CL + t], f);
    Fs[t] = f;
    Fo[t] = f;
  }
  __syncthreads();
  if (wv < C) {
    const float* wc = Wc2 + (size_t)wv * CL;
    float a = dot4(*(const f32x4*)(Fs + 4 * lane), *(const f32x4*)(wc + 4 * lane), 0.f);
    a = dot4(*(const f32x4*)(Fs + 256 + 4 * lane), *(const f32x4*)(wc + 256 + 4 * lane), a);
    a = wave_sum(a);
    if (lane == 0) {
      sl[wv] = a + bc2[wv];
      slide[wv] = a + bc2[wv];
    }
  }
  __syncthreads();
  const long long y = label ? label[0] : -1;
  const bool y_ok = y >= 0 && y < C;
  if (label && t < G) {
    rowloss[t] = y_ok ? lse_of(sub + (size_t)t * C, C) - sub[(size_t)t * C + y] : NAN;
  }
  __syncthreads();
  if (t == 0) {
    const float lse = lse_of(sl, C);
    int best = 0;
    for (int c = 0; c < C; ++c) {
      yprob[c] = expf(sl[c] - lse);
      if (sl[c] > sl[best]) best = c;
    }
    yhat[0] = best;
    if (label) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += rowloss[g];
      losses[0] = s / (float)G;
      losses[1] = y_ok ? lse - sl[y] : NAN;
    }
  }
}

// dsub / dslide / gsub / gslide nullable (zero).  need_t1: d sub, dWc, dbc, dF and the slices' shares of
// dM are written; need_t2: the attCls gradients are written.
__global__ void __launch_bounds__(NT) t2_bwd_kernel(
    const float* __restrict__ M, const float* __restrict__ p2, const float* __restrict__ Z2,
    const float* __restrict__ Fi, const float* __restrict__ sub, const float* __restrict__ slide,
    const long long* __restrict__ label, int G, int D, int C, const float* __restrict__ Wv2,
    const float* __restrict__ Wu2, const float* __restrict__ w2, const float* __restrict__ Wc2,
    const float* __restrict__ dsub, const float* __restrict__ dslide, const float* __restrict__ gsub,
    const float* __restrict__ gslide, int need_t1, int need_t2, float* __restrict__ dsubt, float* __restrict__ dFw,
    float* __restrict__ part, float* __restrict__ dWv2, float* __restrict__ dbv2, float* __restrict__ dWu2,
    float* __restrict__ dbu2, float* __restrict__ dw2, float* __restrict__ db2, float* __restrict__ dWc2,
    float* __restrict__ dbc2, float* __restrict__ dWc, float* __restrict__ dbc) {
  __shared__ __attribute__((aligned(16))) float Wsl[NW * CL];
  __shared__ float dzs[NW * GMAX];
  __shared__ float dsubs[GMAX * CMAX];
  __shared__ __attribute__((aligned(16))) float dFs[CL];
  __shared__ float dsl[CMAX], da2s[GMAX];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const long long y = label ? label[0] : -1;
  // tier 2 in closed form (every workgroup, the same arithmetic)
  if (t < C) {
    float v = dslide ? dslide[t] : 0.f;
    if (gslide && label) v += gslide[0] * (expf(slide[t] - lse_of(slide, C)) - (t == y ? 1.f : 0.f));
    dsl[t] = v;
  }
  __syncthreads();
  if (t < CL) {
    float v = 0.f;
    for (int c = 0; c < C; ++c) v = fmaf(dsl[c], Wc2[(size_t)c * CL + t], v);
    dFs[t] = v;
  }
  __syncthreads();
  for (int g = wv; g < G; g += NW) {
    // sum_g' p2_g' (M_g' . dF) = F . dF: da2_g = p2_g ((M_g - F) . dF), an exact zero for G = 1
    const float* mg = M + (size_t)g * CL;
    const f32x4 x0 = *(const f32x4*)(mg + 4 * lane) - *(const f32x4*)(Fi + 4 * lane);
    const f32x4 x1 = *(const f32x4*)(mg + 256 + 4 * lane) - *(const f32x4*)(Fi + 256 + 4 * lane);
    float a = dot4(x0, *(const f32x4*)(dFs + 4 * lane), 0.f);
    a = dot4(x1, *(const f32x4*)(dFs + 256 + 4 * lane), a);
    a = wave_sum(a);
    if (lane == 0) da2s[g] = a;
  }
  __syncthreads();
  if (wv == 0) {
    // as in tier 1 (t1_bwd_kernel): the rounding residual sum p2 a / sum p2 is taken out
    const float p = lane < G ? p2[lane] : 0.f, a = lane < G ? da2s[lane] : 0.f;
    const float res = wave_sum(p * a) / wave_sum(p);
    if (lane < G) da2s[lane] = p * (a - res);
  }
  __syncthreads();
  // this workgroup's gate columns: wave 2 dd + which owns row d0 + dd of Wv2 (which = 0) / Wu2 (1)
  const int dd = wv >> 1, which = wv & 1, d = blockIdx.x * T2_D + dd;
  const bool on = d < D;
  {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float bacc = 0.f, wacc = 0.f;
    const float wd = on ? w2[d] : 0.f;
    for (int g = 0; g < G; ++g) {
      float dz = 0.f;
      if (on) {
        const float th = tanhf(Z2[(size_t)g * 2 * D + d]), sg = sigmoid_(Z2[(size_t)g * 2 * D + D + d]);
        const GateGrad gz = gate_bwd(da2s[g] * wd, th, sg);
        dz = which == 0 ? gz.a : gz.b;
        wacc = fmaf(da2s[g], th * sg, wacc);
        bacc += dz;
        if (need_t2) {
          const float* mg = M + (size_t)g * CL;
          acc0 += dz * *(const f32x4*)(mg + 4 * lane);
          acc1 += dz * *(const f32x4*)(mg + 256 + 4 * lane);
        }
      }
      if (lane == 0) dzs[wv * GMAX + g] = dz;
    }
    if (need_t2 && on) {
      float* dW = (which == 0 ? dWv2 : dWu2) + (size_t)d * CL;
      *(f32x4*)(dW + 4 * lane) = acc0;
      *(f32x4*)(dW + 256 + 4 * lane) = acc1;
      if (lane == 0) {
        (which == 0 ? dbv2 : dbu2)[d] = bacc;
        if (which == 0) dw2[d] = wacc;
      }
    }
  }
  if (blockIdx.x == 0 && need_t2) {
    if (t == 0) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += da2s[g];
      db2[0] = s;
    }
    if (t < C) dbc2[t] = dsl[t];
    if (t < CL) {
      const float f = Fi[t];
      for (int c = 0; c < C; ++c) dWc2[(size_t)c * CL + t] = dsl[c] * f;
    }
  }
  if (!need_t1) return;                              // uniform over the grid
  // the slice's weight rows, for its share of dM
  for (int e = t; e < NW * (CL / 4); e += NT) {
    const int r = e / (CL / 4), c4 = e % (CL / 4), rd = blockIdx.x * T2_D + (r >> 1);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (rd < D) v = *(const f32x4*)(((r & 1) == 0 ? Wv2 : Wu2) + (size_t)rd * CL + 4 * c4);
    ((f32x4*)Wsl)[e] = v;
  }
  if (blockIdx.x == 0) {
    for (int e = t; e < G * C; e += NT) {
      const int g = e / C, c = e % C;
      float v = dsub ? dsub[e] : 0.f;
      if (gsub && label)
        v += gsub[0] / (float)G * (expf(sub[e] - lse_of(sub + (size_t)g * C, C)) - (c == y ? 1.f : 0.f));
      dsubs[e] = v;
      dsubt[e] = v;
    }
    if (t < CL) dFw[t] = dFs[t];
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (t < CL) {
      for (int c = 0; c < C; ++c) {
        float v = 0.f;
        for (int g = 0; g < G; ++g) v = fmaf(dsubs[g * C + c], M[(size_t)g * CL + t], v);
        dWc[(size_t)c * CL + t] = v;
      }
    }
    if (t < C) {
      float v = 0.f;
      for (int g = 0; g < G; ++g) v += dsubs[g * C + t];
      dbc[t] = v;
    }
  }
  const int gs = t >> 7, col = (t & 127) * 4;
  for (int g = gs; g < G; g += SLICES) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NW; ++r) acc += dzs[r * GMAX + g] * *(const f32x4*)(Wsl + r * CL + col);
    *(f32x4*)(part + ((size_t)blockIdx.x * G + g) * CL + col) = acc;
  }
}

__global__ void __launch_bounds__(NT) t1_bwd_kernel(
    const float* __restrict__ Z, const float* __restrict__ H, const float* __restrict__ p1,
    const float* __restrict__ M, const float* __restrict__ p2, const float* __restrict__ dFw,
    const float* __restrict__ part, int nb, const float* __restrict__ dsubt, const float* __restrict__ Wc,
    const float* __restrict__ w, int G, int S, int D, int C, float* __restrict__ dZ, float* __restrict__ dH,
    float* __restrict__ dwpart, float* __restrict__ dbpart) {
  __shared__ __attribute__((aligned(16))) float dMs[CL];
  __shared__ __attribute__((aligned(16))) float ws[DMAX];
  __shared__ __attribute__((aligned(16))) float buf[NW * DMAX];
  __shared__ float dps[SMAX];
  __shared__ float dbs[NW];
  __shared__ float red[NW];
  const int g = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  for (int d = t; d < D; d += NT) ws[d] = w[d];
  if (t < CL) {
    float v = p2[g] * dFw[t];
    for (int b = 0; b < nb; ++b) v += part[((size_t)b * G + g) * CL + t];
    for (int c = 0; c < C; ++c) v = fmaf(dsubt[(size_t)g * C + c], Wc[(size_t)c * CL + t], v);
    dMs[t] = v;
  }
  __syncthreads();
  // the softmax correction sum_j p_j (h_j . dM) is M_g . dM: da_i = p_i ((h_i - M_g) . dM), which is an
  // exact zero for a pseudo-bag of one row and cancels less than h_i . dM - M_g . dM elsewhere
  const float* mg = M + (size_t)g * CL;
  const f32x4 c0 = *(const f32x4*)(mg + 4 * lane), c1 = *(const f32x4*)(mg + 256 + 4 * lane);
  const float* Zg = Z + (size_t)g * S * 2 * D;
  const float* Hg = H + (size_t)g * S * CL;
  float* dZg = dZ + (size_t)g * S * 2 * D;
  float* dHg = dH + (size_t)g * S * CL;
  const f32x4 m0 = *(const f32x4*)(dMs + 4 * lane), m1 = *(const f32x4*)(dMs + 256 + 4 * lane);
  // phase 1, the only read of the h rows: dps[j] = (h_j - M_g) . dM
#pragma unroll 1
  for (int j = wv; j < S; j += NW) {
    const float* h = Hg + (size_t)j * CL;
    const f32x4 h0 = *(const f32x4*)(h + 4 * lane), h1 = *(const f32x4*)(h + 256 + 4 * lane);
    const float dp = wave_sum(dot4(h1 - c1, m1, dot4(h0 - c0, m0, 0.f)));
    if (lane == 0) dps[j] = dp;
  }
  __syncthreads();
  // sum_j p_j dps[j] is zero in exact arithmetic; in fp32 it is the rounding of M_g and of sum p = 1.
  // Taking it out (res = sum p dps / sum p) makes the da of a pseudo-bag add up to zero as the exact ones do
  float num = 0.f, den = 0.f;
  for (int j = t; j < S; j += NT) {
    const float p = p1[(size_t)g * S + j];
    num = fmaf(p, dps[j], num);
    den += p;
  }
  num = block_reduce<false, NW>(num, red);
  den = block_reduce<false, NW>(den, red);
  const float res = num / den;
  f32x4 dwacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float dbacc = 0.f;
#pragma unroll 1
  for (int j = wv; j < S; j += NW) {
    const float p = p1[(size_t)g * S + j];
    const float da = p * (dps[j] - res);
    dbacc += da;
    float* gh = dHg + (size_t)j * CL;
    *(f32x4*)(gh + 4 * lane) = p * m0;
    *(f32x4*)(gh + 256 + 4 * lane) = p * m1;
    const float* z = Zg + (size_t)j * 2 * D;
    float* gz = dZg + (size_t)j * 2 * D;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int d = 4 * lane + 256 * ch;
      if (d < D) {
        const f32x4 za = *(const f32x4*)(z + d), zb = *(const f32x4*)(z + D + d), wd = *(const f32x4*)(ws + d);
        f32x4 ga, gb;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float th = tanhf(za[u]), sg = sigmoid_(zb[u]);
          const GateGrad gz4 = gate_bwd(da * wd[u], th, sg);
          ga[u] = gz4.a;
          gb[u] = gz4.b;
          dwacc[ch][u] = fmaf(da, th * sg, dwacc[ch][u]);
        }
        *(f32x4*)(gz + d) = ga;
        *(f32x4*)(gz + D + d) = gb;
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const int d = 4 * lane + 256 * ch;
    if (d < D) *(f32x4*)(buf + wv * DMAX + d) = dwacc[ch];
  }
  if (lane == 0) dbs[wv] = dbacc;
  __syncthreads();
  for (int d = t; d < D; d += NT) {
    float v = buf[d];
#pragma unroll
    for (int q = 1; q < NW; ++q) v += buf[q * DMAX + d];
    dwpart[(size_t)g * D + d] = v;
  }
  if (t == 0) {
    float v = dbs[0];
    for (int q = 1; q < NW; ++q) v += dbs[q];
    dbpart[g] = v;
  }
}

__global__ void __launch_bounds__(256) t1_reduce_kernel(const float* __restrict__ dwpart,
                                                        const float* __restrict__ dbpart, int G, int D,
                                                        float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < D) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += dwpart[(size_t)g * D + e];
    dw[e] = s;
  } else if (e == D) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += dbpart[g];
    db[0] = s;
  }
}

const char* check_shape(int G, int S, int L, int D, int C) {
  if (L != CL) return "dtfd: m_dim must be 512";
  if (D < 4 || D % 4 != 0 || D > DMAX) return "dtfd: D must be a multiple of 4, <= 512";
  if (C < 1 || C > CMAX) return "dtfd: n_classes must be in [1, 8]";
  if (S < 1 || S > SMAX) return "dtfd: bag_size must be in [1, 1024]";
  if (G < 1 || G > GMAX) return "dtfd: the number of pseudo-bags must be in [1, 64]";
  return nullptr;
}

int t2_slices(int D) { return (D + T2_D - 1) / T2_D; }

}  // namespace

extern "C" int tm_dtfd_fwd(const float* Z, const float* H, int G, int S, int L, int D, int C, const float* w,
                           const float* b, const float* Wc, const float* bc, const float* Wv2, const float* bv2,
                           const float* Wu2, const float* bu2, const float* w2, const float* b2, const float* Wc2,
                           const float* bc2, const long long* label, float* p1, float* M, float* sub, float* cam,
                           float* Z2, float* p2, float* F, float* slide, float* losses, float* yprob,
                           long long* yhat, void* stream) {
  const char* bad = check_shape(G, S, L, D, C);
  TM_REQUIRE(bad == nullptr, bad);
  TM_REQUIRE(Z && H && w && b && Wc && bc && Wv2 && bv2 && Wu2 && bu2 && w2 && b2 && Wc2 && bc2, "dtfd: inputs missing");
  TM_REQUIRE(p1 && M && sub && Z2 && p2 && F && slide && yprob && yhat && (!label || losses), "dtfd: outputs missing");
  hipStream_t st = (hipStream_t)stream;
  t1_fwd_kernel<<<G, NT, 0, st>>>(Z, H, S, D, C, w, b, Wc, bc, p1, M, sub, cam);
  t2_fwd_kernel<<<1, NT, 0, st>>>(M, G, D, C, Wv2, bv2, Wu2, bu2, w2, b2, Wc2, bc2, sub, label, Z2, p2, F, slide,
                                  losses, yprob, yhat);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_dtfd_bwd_workspace(int G, int D, int C) {
  if (check_shape(G, 1, CL, D, C) != nullptr) return 0;
  return ((long long)GMAX * CMAX + CL + (long long)G * D + GMAX + (long long)t2_slices(D) * G * CL) *
         (long long)sizeof(float);
}

extern "C" int tm_dtfd_bwd(const float* Z, const float* H, const float* p1, const float* M, const float* p2,
                           const float* Z2, const float* F, const float* sub, const float* slide,
                           const long long* label, int G, int S, int L, int D, int C, const float* w, const float* Wc,
                           const float* Wv2, const float* Wu2, const float* w2, const float* Wc2, const float* dsub,
                           const float* dslide, const float* gsub, const float* gslide, int need_t1, int need_t2,
                           float* work, float* dZ, float* dH, float* dw, float* db, float* dWc, float* dbc,
                           float* dWv2, float* dbv2, float* dWu2, float* dbu2, float* dw2, float* db2, float* dWc2,
                           float* dbc2, void* stream) {
  const char* bad = check_shape(G, S, L, D, C);
  TM_REQUIRE(bad == nullptr, bad);
  if (!need_t1 && !need_t2) return 0;
  TM_REQUIRE(M && p2 && Z2 && F && sub && slide && Wv2 && Wu2 && w2 && Wc2 && work, "dtfd: saved tensors missing");
  TM_REQUIRE(!need_t1 || (Z && H && p1 && w && Wc && dZ && dH && dw && db && dWc && dbc), "dtfd: tier-1 buffers missing");
  TM_REQUIRE(!need_t2 || (dWv2 && dbv2 && dWu2 && dbu2 && dw2 && db2 && dWc2 && dbc2), "dtfd: tier-2 buffers missing");
  hipStream_t st = (hipStream_t)stream;
  const int nb = t2_slices(D);
  float* dsubt = work;                          // [G][C]
  float* dFw = dsubt + GMAX * CMAX;             // [CL]
  float* dwpart = dFw + CL;                     // [G][D]
  float* dbpart = dwpart + (size_t)G * D;       // [G]
  float* part = dbpart + GMAX;                  // [nb][G][CL], 16-B aligned rows
  t2_bwd_kernel<<<nb, NT, 0, st>>>(M, p2, Z2, F, sub, slide, label, G, D, C, Wv2, Wu2, w2, Wc2, dsub, dslide, gsub,
                                   gslide, need_t1, need_t2, dsubt, dFw, part, dWv2, dbv2, dWu2, dbu2, dw2, db2, dWc2,
                                   dbc2, dWc, dbc);
  if (need_t1) {
    t1_bwd_kernel<<<G, NT, 0, st>>>(Z, H, p1, M, p2, dFw, part, nb, dsubt, Wc, w, G, S, D, C, dZ, dH, dwpart, dbpart);
    t1_reduce_kernel<<<(D + 1 + 255) / 256, 256, 0, st>>>(dwpart, dbpart, G, D, dw, db);
  }
  TM_CHECK_LAUNCH();
  return 0;
}
