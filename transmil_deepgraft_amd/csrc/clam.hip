// CLAM_MB (code/models/model_clam.py:195-268): K-branch gated attention pooling with per-class
// two-sided top-k instance selection and the instance-classifier loss, fp32, the non-GEMM part.
//   g_i     = tanh(Z[i, :D]) * sigmoid(Z[i, D:])           Z = h [Wa;Wb]^T + [ba;bb] (the caller's GEMM)
//   a[c,i]  = Wc[c] . g_i + bc[c]                          A_raw [K, N]
//   p[c,:]  = softmax_N(a[c,:]) ;  M = p h  [K, L] ;  logits[c] = wcls_c . M[c] + bcls_c
//   instance evaluation (label y on the device): class y takes the k largest scores of a[y,:]
//   (descending, targets 1) and the k smallest (ascending, targets 0); with subtyping every other
//   class takes its k largest (targets 0).  il = h[idx] W_ic^T + b_ic, loss_c = mean CE, the loss is
//   the sum over the evaluated classes (divided by K with subtyping).  Among equal scores the lower
//   instance index is taken first, on both sides.
// Forward, two stream-ordered launches:
//   rows_fwd_kernel   grid over blocks of RB rows.  A wave per row computes g and the K scores from one
//                     read of the Z row (16-byte loads); the block then takes its own maximum m_blk[c]
//                     and sum s_blk[c] = sum exp(a - m_blk) and adds exp(a - m_blk) h_i for all K
//                     classes from one read of each h row (one f32x4 accumulator per class).
//   finalize_kernel   workgroup c < K merges the block partials flash-style (m = max m_blk, each
//                     partial weighted by exp(m_blk - m)) and writes stats[c] = {m, s}, M[c], logits[c];
//                     with a label, workgroup K selects per evaluated class by k rounds of "the next
//                     pair after the last one taken" over A_raw[c,:], gathers the rows of h and writes
//                     il's cross entropy, predictions, targets and d loss / d il.
//   No exp of an unshifted score anywhere, and no score-sized statistics pass.
// Backward, a head kernel, one row pass and the sum of the row pass's block partials:
//   bwd_head_kernel   dM[c] = dlogits[c] wcls_c, dwcls, dbcls, r[c] = M[c] . dM[c]
//                     (= sum_j p_j dp_j, the softmax correction, so no extra pass over h); the instance
//                     classifiers' gradients and the list of (row, [L] vector) contributions to dh
//   rows_bwd_kernel   p = exp(a - m) / s from A_raw and stats; da[c,i] = p (h_i . dM[c] - r[c]);
//                     dg = sum_c da Wc[c]; dZ through tanh / sigmoid; dh_i = sum_c p dM[c] plus the listed
//                     contributions of row i in list order; block partials of dWc / dbc
//   bwd_reduce_kernel dWc, dbc = the block partials added in block order
// No float atomics: every sum is a fixed tree or an index-ordered loop, so results repeat bitwise.
#include "common.h"
#include "mil_common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int CL = 512;           // L: width of h (size_dict[*][1] of the model)
constexpr int KMAX = 8;           // classes (attention branches)
constexpr int DMAX = 512;         // D: gate width
constexpr int SMAX = 32;          // k_sample
constexpr int RB_MAX = 512;       // rows per row-pass block
constexpr int FIN_THREADS = 1024;
constexpr int FIN_WAVES = FIN_THREADS / 64;
constexpr int FIN_SLICES = FIN_THREADS / (CL / 4);   // 8 groups of 128 f32x4 columns

// Forward row pass, compiled for KT = 2, 4, 8 classes (the smallest KT >= K: the per-class
// accumulators are registers, classes K..KT-1 carry zero weights and are never stored).
// LDS: wcs [KT][D] | sc [KT][RB] (scores, then exp(a - m_blk)) | comb [KT][CL].
// part == nullptr: scores only (attention_only).
template <int KT>
__global__ void __launch_bounds__(256) rows_fwd_kernel(const float* __restrict__ Z, const float* __restrict__ H,
                                                       int N, int D, int K, int RB, const float* __restrict__ Wc,
                                                       const float* __restrict__ bc, float* __restrict__ A_raw,
                                                       float* __restrict__ mb, float* __restrict__ sb,
                                                       float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wcs = sm;
  float* sc = wcs + KT * D;
  float* comb = sc + KT * RB;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int r0 = blockIdx.x * RB, nrows = min(N - r0, RB);
  for (int e = t; e < KT * D; e += 256) wcs[e] = e < K * D ? Wc[e] : 0.f;
  for (int e = K * RB + t; e < KT * RB; e += 256) sc[e] = 0.f;
  __syncthreads();
#pragma unroll 1
  for (int j = wv; j < nrows; j += 4) {
    const float* z = Z + (size_t)(r0 + j) * 2 * D;
    float acc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) acc[c] = 0.f;
    for (int d = 4 * lane; d < D; d += 256) {
      const f32x4 za = *(const f32x4*)(z + d), zb = *(const f32x4*)(z + D + d);
      const f32x4 g = gate(za, zb);
#pragma unroll
      for (int c = 0; c < KT; ++c) acc[c] = dot4(g, *(const f32x4*)(wcs + c * D + d), acc[c]);
    }
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      const float v = wave_sum(acc[c]);
      if (lane == 0 && c < K) {
        const float a = v + bc[c];
        sc[c * RB + j] = a;
        A_raw[(size_t)c * N + r0 + j] = a;
      }
    }
  }
  if (part == nullptr) return;
  __syncthreads();
  // block-local softmax statistics: wave c % 4 takes class c
  for (int c = wv; c < K; c += 4) {
    float* s = sc + c * RB;
    float m = -INFINITY;
    for (int j = lane; j < nrows; j += 64) m = fmaxf(m, s[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nrows; j += 64) {
      const float e = expf(s[j] - m);
      s[j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) {
      mb[(size_t)blockIdx.x * K + c] = m;
      sb[(size_t)blockIdx.x * K + c] = sum;
    }
  }
  __syncthreads();
  // pooled partials: threads 0..127 take the even rows, 128..255 the odd ones, four rows in flight
  const int half = t >> 7, col = (t & 127) * 4;
  f32x4 acc[KT];
#pragma unroll
  for (int c = 0; c < KT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* hb = H + (size_t)r0 * CL + col;
#pragma unroll 1
  for (int j0 = half; j0 < nrows; j0 += 8) {
    f32x4 h[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) h[u] = *(const f32x4*)(hb + (size_t)min(j0 + 2 * u, nrows - 1) * CL);   // in bounds
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 2 * u;
      const bool on = j < nrows;
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        const float e = on ? sc[c * RB + min(j, nrows - 1)] : 0.f;
        acc[c] += e * h[u];
      }
    }
  }
  if (half == 1) {
#pragma unroll
    for (int c = 0; c < KT; ++c) *(f32x4*)(comb + c * CL + col) = acc[c];
  }
  __syncthreads();
  if (half == 0) {
    float* out = part + (size_t)blockIdx.x * K * CL + col;
#pragma unroll
    for (int c = 0; c < KT; ++c)
      if (c < K) *(f32x4*)(out + c * CL) = acc[c] + *(const f32x4*)(comb + c * CL + col);
  }
}

// k rounds over one class's N scores: round r takes, on each side, the first pair in that side's
// order that comes after the pair taken in round r - 1.  sel_hi / sel_lo [k] (LDS) receive the indices.
TM_DEV void select_rounds(const float* __restrict__ a, int N, int k, Pair (*red)[2][FIN_WAVES], int* sel_hi,
                          int* sel_lo) {
  Pair last_hi = {INFINITY, -1}, last_lo = {-INFINITY, -1};
  for (int r = 0; r < k; ++r) {
    Pair hi = {-INFINITY, INT_MAX}, lo = {INFINITY, INT_MAX};
    for (int i = threadIdx.x; i < N; i += FIN_THREADS) {
      const float v = a[i];
      if (before_max(last_hi.v, last_hi.i, Pair{v, i}) && before_max(v, i, hi)) hi = {v, i};
      if (before_min(last_lo.v, last_lo.i, Pair{v, i}) && before_min(v, i, lo)) lo = {v, i};
    }
    const PairLoHi got = select_round_tail<FIN_WAVES>(lo, hi, red[r & 1]);   // two buffers: one barrier per round
    last_hi = got.hi;
    last_lo = got.lo;
    if (threadIdx.x == 0) {
      sel_hi[r] = select_clamp(got.hi.i, N);
      sel_lo[r] = select_clamp(got.lo.i, N);
    }
  }
  __syncthreads();
}

// Workgroups [0, K): merge of the block partials of class c.  Workgroup K (only with a label): the
// instance evaluation of every evaluated class, one after the other.
__global__ void __launch_bounds__(FIN_THREADS) finalize_kernel(
    const float* __restrict__ mb, const float* __restrict__ sb, const float* __restrict__ part, int nblk,
    const float* __restrict__ A_raw, const float* __restrict__ H, int N, int K, const float* __restrict__ Wcls,
    const float* __restrict__ bcls, const float* __restrict__ Wic, const float* __restrict__ bic,
    const long long* __restrict__ label, int k, int subtyping, float* __restrict__ stats, float* __restrict__ M,
    float* __restrict__ logits, float* __restrict__ inst_loss, int* __restrict__ idx, int* __restrict__ preds,
    int* __restrict__ targets, float* __restrict__ dil) {
  __shared__ __attribute__((aligned(16))) float acc_s[FIN_SLICES * CL];
  __shared__ float red[FIN_WAVES];
  __shared__ Pair pred[2][2][FIN_WAVES];
  __shared__ int sel_hi[SMAX], sel_lo[SMAX], rows[2 * SMAX];
  __shared__ float il[2 * SMAX][2], lossj[2 * SMAX];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < K) {
    const int c = blockIdx.x;
    float m = -INFINITY;
    for (int b = t; b < nblk; b += FIN_THREADS) m = fmaxf(m, mb[(size_t)b * K + c]);
    m = block_reduce<true>(m, red);
    float s = 0.f;
    for (int b = t; b < nblk; b += FIN_THREADS) s += sb[(size_t)b * K + c] * expf(mb[(size_t)b * K + c] - m);
    s = block_reduce<false>(s, red);
    // slice q adds the blocks q, q + 8, ... in order; the eight slices are then added in order
    const int slice = t >> 7, col = (t & 127) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = slice; b < nblk; b += FIN_SLICES)
      acc += expf(mb[(size_t)b * K + c] - m) * *(const f32x4*)(part + ((size_t)b * K + c) * CL + col);
    *(f32x4*)(acc_s + slice * CL + col) = acc;
    __syncthreads();
    float prod = 0.f;
    if (t < CL) {
      float v = acc_s[t];
#pragma unroll
      for (int q = 1; q < FIN_SLICES; ++q) v += acc_s[q * CL + t];
      v /= s;
      M[(size_t)c * CL + t] = v;
      prod = v * Wcls[(size_t)c * CL + t];
    }
    prod = block_reduce<false>(prod, red);
    if (t == 0) {
      logits[c] = prod + bcls[c];
      stats[2 * c] = m;
      stats[2 * c + 1] = s;
    }
    return;
  }
  // instance evaluation
  const int k2 = 2 * k, wave = t >> 6, lane = t & 63;
  for (int e = t; e < K * k2; e += FIN_THREADS) {
    idx[e] = -1;
    preds[e] = -1;
    targets[e] = -1;
    dil[2 * e] = 0.f;
    dil[2 * e + 1] = 0.f;
  }
  const long long y = label[0];
  float total = 0.f;        // thread 0's
  for (int c = 0; c < K; ++c) {
    const bool pos = c == y;
    if (!pos && !subtyping) continue;
    select_rounds(A_raw + (size_t)c * N, N, k, pred, sel_hi, sel_lo);
    const int nsel = pos ? k2 : k;
    if (t < nsel) rows[t] = t < k ? sel_hi[t] : sel_lo[t - k];
    __syncthreads();
    for (int e = wave; e < 2 * nsel; e += FIN_WAVES) {      // a wave per (selected row, output)
      const int j = e >> 1, o = e & 1;
      const float* h = H + (size_t)rows[j] * CL;
      const float* w = Wic + ((size_t)c * 2 + o) * CL;
      float a = dot4(*(const f32x4*)(h + 4 * lane), *(const f32x4*)(w + 4 * lane), 0.f);
      a = dot4(*(const f32x4*)(h + 256 + 4 * lane), *(const f32x4*)(w + 256 + 4 * lane), a);
      a = wave_sum(a);
      if (lane == 0) il[j][o] = a + bic[c * 2 + o];
    }
    __syncthreads();
    if (t < nsel) {
      const int tgt = (pos && t < k) ? 1 : 0;
      const float l0 = il[t][0], l1 = il[t][1];
      const float lse = lse_of(il[t], 2);
      const float scale = (subtyping ? 1.f / (float)K : 1.f) / (float)nsel;
      lossj[t] = lse - (tgt ? l1 : l0);
      const int e = c * k2 + t;
      dil[2 * e] = (expf(l0 - lse) - (tgt ? 0.f : 1.f)) * scale;
      dil[2 * e + 1] = (expf(l1 - lse) - (tgt ? 1.f : 0.f)) * scale;
      idx[e] = rows[t];
      preds[e] = l1 > l0 ? 1 : 0;
      targets[e] = tgt;
    }
    __syncthreads();
    if (t == 0) {
      float s = 0.f;
      for (int j = 0; j < nsel; ++j) s += lossj[j];
      total += s / (float)nsel;
    }
    __syncthreads();
  }
  if (t == 0) inst_loss[0] = subtyping ? total / (float)K : total;
}

// One workgroup of CL threads (thread t: column t).  dlogits / gloss nullable (zero).  idx == nullptr:
// no instance part.
__global__ void __launch_bounds__(CL) bwd_head_kernel(
    const float* __restrict__ dlogits, const float* __restrict__ gloss, const float* __restrict__ M,
    const float* __restrict__ H, int N, int K, const float* __restrict__ Wcls, const float* __restrict__ Wic,
    const int* __restrict__ idx, const float* __restrict__ dil, int k2, float* __restrict__ dM,
    float* __restrict__ rv, float* __restrict__ dWcls, float* __restrict__ dbcls, float* __restrict__ dWic,
    float* __restrict__ dbic, int* __restrict__ lrow, float* __restrict__ lvec) {
  __shared__ float red[CL / 64];
  const int t = threadIdx.x;
  for (int c = 0; c < K; ++c) {
    const float dl = dlogits ? dlogits[c] : 0.f;
    const float m = M[(size_t)c * CL + t], g = dl * Wcls[(size_t)c * CL + t];
    dM[(size_t)c * CL + t] = g;
    dWcls[(size_t)c * CL + t] = dl * m;
    const float r = block_reduce<false>(m * g, red);
    if (t == 0) {
      rv[c] = r;
      dbcls[c] = dl;
    }
  }
  if (idx == nullptr) return;
  const float gl = gloss ? gloss[0] : 0.f;
  for (int c = 0; c < K; ++c) {
    float a0 = 0.f, a1 = 0.f;
    for (int j = 0; j < k2; ++j) {           // list order
      const int e = c * k2 + j, row = idx[e];
      const bool on = row >= 0 && row < N;
      const float d0 = on ? gl * dil[2 * e] : 0.f, d1 = on ? gl * dil[2 * e + 1] : 0.f;
      const float w0 = Wic[((size_t)c * 2) * CL + t], w1 = Wic[((size_t)c * 2 + 1) * CL + t];
      if (on) {
        const float h = H[(size_t)row * CL + t];
        a0 = fmaf(d0, h, a0);
        a1 = fmaf(d1, h, a1);
      }
      lvec[(size_t)e * CL + t] = d0 * w0 + d1 * w1;
      if (t == 0) lrow[e] = on ? row : -1;
    }
    dWic[((size_t)c * 2) * CL + t] = a0;
    dWic[((size_t)c * 2 + 1) * CL + t] = a1;
  }
  if (t < 2 * K) {
    const int c = t >> 1, o = t & 1;
    float a = 0.f;
    for (int j = 0; j < k2; ++j) {
      const int e = c * k2 + j;
      if (idx[e] >= 0 && idx[e] < N) a += gl * dil[2 * e + o];
    }
    dbic[t] = a;
  }
}

// Backward row pass: a wave per row, RB rows per workgroup; KT as in the forward row pass (classes
// K..KT-1 carry zero dM, Wc and da).
// LDS: dMs [KT][CL] | wcs [KT][D] | buf [4][DMAX] | lrows [nlist] | dbs [4][KMAX]
template <int KT>
__global__ void __launch_bounds__(256) rows_bwd_kernel(
    const float* __restrict__ Z, const float* __restrict__ H, const float* __restrict__ A_raw,
    const float* __restrict__ stats, int N, int D, int K, int RB, const float* __restrict__ Wc,
    const float* __restrict__ dM, const float* __restrict__ rv, const int* __restrict__ lrow,
    const float* __restrict__ lvec, int nlist, float* __restrict__ dZ, float* __restrict__ dH,
    float* __restrict__ dwc_part, float* __restrict__ dbc_part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dMs = sm;
  float* wcs = dMs + KT * CL;
  float* buf = wcs + KT * D;
  int* lrows = (int*)(buf + 4 * DMAX);
  float* dbs = (float*)(lrows + ((nlist + 3) & ~3));
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int r0 = blockIdx.x * RB, r1 = min(N, r0 + RB);
  for (int e = t; e < KT * CL; e += 256) dMs[e] = e < K * CL ? dM[e] : 0.f;
  for (int e = t; e < KT * D; e += 256) wcs[e] = e < K * D ? Wc[e] : 0.f;
  for (int e = t; e < nlist; e += 256) lrows[e] = lrow[e];
  __syncthreads();
  float mc[KT], inv[KT], rc[KT], dbacc[KT];
  f32x4 dwacc[2][KT];
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    mc[c] = c < K ? stats[2 * c] : 0.f;
    inv[c] = c < K ? 1.f / stats[2 * c + 1] : 0.f;       // 0: classes K..KT-1 get p = 0
    rc[c] = c < K ? rv[c] : 0.f;
    dbacc[c] = 0.f;
    dwacc[0][c] = dwacc[1][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 1
  for (int i = r0 + wv; i < r1; i += 4) {
    const float* h = H + (size_t)i * CL;
    const f32x4 h0 = *(const f32x4*)(h + 4 * lane), h1 = *(const f32x4*)(h + 256 + 4 * lane);
    f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
    float da[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      const f32x4 m0 = *(const f32x4*)(dMs + c * CL + 4 * lane), m1 = *(const f32x4*)(dMs + c * CL + 256 + 4 * lane);
      const float dp = wave_sum(dot4(h1, m1, dot4(h0, m0, 0.f)));
      const float a = A_raw[(size_t)min(c, K - 1) * N + i];                 // in bounds for every c
      const float p = c < K ? expf(a - mc[c]) * inv[c] : 0.f;
      da[c] = p * (dp - rc[c]);
      dbacc[c] += da[c];
      g0 += p * m0;
      g1 += p * m1;
    }
    for (int e0 = 0; e0 < nlist; e0 += 64) {          // the instance classifiers' contributions, list order
      const int e = e0 + lane;
      unsigned long long hit = __ballot(e < nlist && lrows[e] == i);
      while (hit) {
        const int b = __ffsll((long long)hit) - 1;
        hit &= hit - 1;
        const float* v = lvec + (size_t)(e0 + b) * CL;
        g0 += *(const f32x4*)(v + 4 * lane);
        g1 += *(const f32x4*)(v + 256 + 4 * lane);
      }
    }
    float* gh = dH + (size_t)i * CL;
    *(f32x4*)(gh + 4 * lane) = g0;
    *(f32x4*)(gh + 256 + 4 * lane) = g1;
    const float* z = Z + (size_t)i * 2 * D;
    float* gz = dZ + (size_t)i * 2 * D;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int d = 4 * lane + 256 * ch;
      if (d < D) {
        const f32x4 za = *(const f32x4*)(z + d), zb = *(const f32x4*)(z + D + d);
        f32x4 dg = {0.f, 0.f, 0.f, 0.f}, th, sg, gg;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          th[u] = tanhf(za[u]);
          sg[u] = sigmoid_(zb[u]);
          gg[u] = th[u] * sg[u];
        }
#pragma unroll
        for (int c = 0; c < KT; ++c) {
          dg += da[c] * *(const f32x4*)(wcs + c * D + d);
          dwacc[ch][c] += da[c] * gg;
        }
        f32x4 ga, gb;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const GateGrad gz4 = gate_bwd(dg[u], th[u], sg[u]);
          ga[u] = gz4.a;
          gb[u] = gz4.b;
        }
        *(f32x4*)(gz + d) = ga;
        *(f32x4*)(gz + D + d) = gb;
      }
    }
  }
  // the four waves' dWc / dbc partials, added in wave order
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int d = 4 * lane + 256 * ch;
      if (d < D) *(f32x4*)(buf + wv * DMAX + d) = dwacc[ch][c];
    }
    if (lane == 0) dbs[wv * KMAX + c] = dbacc[c];
    __syncthreads();
    if (c < K) {
      for (int d = t; d < D; d += 256)
        dwc_part[((size_t)blockIdx.x * K + c) * D + d] = buf[d] + buf[DMAX + d] + buf[2 * DMAX + d] + buf[3 * DMAX + d];
    }
  }
  if (t < K)
    dbc_part[(size_t)blockIdx.x * K + t] = dbs[t] + dbs[KMAX + t] + dbs[2 * KMAX + t] + dbs[3 * KMAX + t];
}

// dWc[e] / dbc[c] = the block partials added in block order
__global__ void __launch_bounds__(256) bwd_reduce_kernel(const float* __restrict__ dwc_part,
                                                         const float* __restrict__ dbc_part, int nblk, int KD, int K,
                                                         float* __restrict__ dWc, float* __restrict__ dbc) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < KD) {
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += dwc_part[(size_t)b * KD + e];
    dWc[e] = s;
  } else if (e < KD + K) {
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += dbc_part[(size_t)b * K + e - KD];
    dbc[e - KD] = s;
  }
}

// rows per row-pass workgroup: at most 512 workgroups up to N = 262144, at least 16 rows each
int rows_per_block(int N) {
  const int rb = ((N + 511) / 512 + 15) / 16 * 16;
  return rb < 16 ? 16 : (rb > RB_MAX ? RB_MAX : rb);
}
int nblk_of(int N) {
  const int rb = rows_per_block(N);
  return (N + rb - 1) / rb;
}

const char* check_shape(int N, int L, int D, int K) {
  if (N < 1) return "clam: N must be >= 1";
  if (L != CL) return "clam: L must be 512";
  if (D < 4 || D % 4 != 0 || D > DMAX) return "clam: D must be a multiple of 4, <= 512";
  if (K < 1 || K > KMAX) return "clam: n_classes must be in [1, 8]";
  return nullptr;
}

int kt_of(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : 8; }

void launch_rows_fwd(const float* Z, const float* H, int N, int D, int K, const float* Wc, const float* bc,
                     float* A_raw, float* mb, float* sb, float* part, hipStream_t st) {
  const int RB = rows_per_block(N), nblk = nblk_of(N), KT = kt_of(K);
  const size_t lds = (size_t)KT * (D + RB + CL) * sizeof(float);      // <= 48 KiB
  if (KT == 2) rows_fwd_kernel<2><<<nblk, 256, lds, st>>>(Z, H, N, D, K, RB, Wc, bc, A_raw, mb, sb, part);
  else if (KT == 4) rows_fwd_kernel<4><<<nblk, 256, lds, st>>>(Z, H, N, D, K, RB, Wc, bc, A_raw, mb, sb, part);
  else rows_fwd_kernel<8><<<nblk, 256, lds, st>>>(Z, H, N, D, K, RB, Wc, bc, A_raw, mb, sb, part);
}

}  // namespace

extern "C" long long tm_clam_fwd_workspace(int N, int K) {
  if (N < 1 || K < 1 || K > KMAX) return 0;
  return (long long)nblk_of(N) * K * (2 + CL) * (long long)sizeof(float);
}

extern "C" int tm_clam_scores(const float* Z, int N, int D, int K, const float* Wc, const float* bc, float* A_raw,
                              void* stream) {
  const char* bad = check_shape(N, CL, D, K);
  TM_REQUIRE(bad == nullptr, bad);
  launch_rows_fwd(Z, nullptr, N, D, K, Wc, bc, A_raw, nullptr, nullptr, nullptr, (hipStream_t)stream);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_clam_fwd(const float* Z, const float* H, int N, int L, int D, int K, const float* Wc,
                           const float* bc, const float* Wcls, const float* bcls, const float* Wic, const float* bic,
                           const long long* label, int k_sample, int subtyping, float* work, float* A_raw,
                           float* stats, float* M, float* logits, float* inst_loss, int* idx, int* preds,
                           int* targets, float* dil, void* stream) {
  const char* bad = check_shape(N, L, D, K);
  TM_REQUIRE(bad == nullptr, bad);
  if (label) {
    TM_REQUIRE(k_sample >= 1 && k_sample <= SMAX, "clam: k_sample must be in [1, 32]");
    TM_REQUIRE(N >= k_sample, "clam: N must be >= k_sample (selected index out of range)");
    TM_REQUIRE(Wic && bic && inst_loss && idx && preds && targets && dil, "clam: instance evaluation buffers missing");
  }
  hipStream_t st = (hipStream_t)stream;
  const int nblk = nblk_of(N);
  float* part = work;                              // [nblk][K][CL], 16-B aligned rows
  float* mb = part + (size_t)nblk * K * CL;        // [nblk][K]
  float* sb = mb + (size_t)nblk * K;               // [nblk][K]
  launch_rows_fwd(Z, H, N, D, K, Wc, bc, A_raw, mb, sb, part, st);
  finalize_kernel<<<K + (label ? 1 : 0), FIN_THREADS, 0, st>>>(mb, sb, part, nblk, A_raw, H, N, K, Wcls, bcls, Wic,
                                                               bic, label, k_sample, subtyping, stats, M, logits,
                                                               inst_loss, idx, preds, targets, dil);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_clam_bwd_workspace(int N, int D, int K, int k_sample) {
  if (N < 1 || K < 1 || K > KMAX || D < 1 || D > DMAX || k_sample < 0 || k_sample > SMAX) return 0;
  const long long nlist = (long long)K * 2 * k_sample, npad = (nlist + 3) & ~3LL;
  return ((long long)K * CL + KMAX + npad + nlist * CL + (long long)nblk_of(N) * K * (D + 1)) * (long long)sizeof(float);
}

extern "C" int tm_clam_bwd(const float* Z, const float* H, const float* A_raw, const float* stats, const float* M,
                           int N, int L, int D, int K, const float* Wc, const float* Wcls, const float* Wic,
                           const int* idx, const float* dil, int k_sample, const float* dlogits, const float* dloss,
                           float* work, float* dZ, float* dH, float* dWc, float* dbc, float* dWcls, float* dbcls,
                           float* dWic, float* dbic, void* stream) {
  const char* bad = check_shape(N, L, D, K);
  TM_REQUIRE(bad == nullptr, bad);
  if (idx) {
    TM_REQUIRE(k_sample >= 1 && k_sample <= SMAX, "clam: k_sample must be in [1, 32]");
    TM_REQUIRE(Wic && dil && dWic && dbic, "clam: instance evaluation buffers missing");
  }
  hipStream_t st = (hipStream_t)stream;
  const int RB = rows_per_block(N), nblk = nblk_of(N);
  const int nlist = idx ? K * 2 * k_sample : 0;
  float* dM = work;
  float* rv = dM + (size_t)K * CL;
  int* lrow = (int*)(rv + KMAX);
  float* lvec = (float*)(lrow + ((nlist + 3) & ~3));     // 16-B aligned rows
  float* dwc_part = lvec + (size_t)nlist * CL;
  float* dbc_part = dwc_part + (size_t)nblk * K * D;
  bwd_head_kernel<<<1, CL, 0, st>>>(dlogits, dloss, M, H, N, K, Wcls, Wic, idx, dil, 2 * k_sample, dM, rv, dWcls,
                                    dbcls, dWic, dbic, lrow, lvec);
  const int KT = kt_of(K);
  const size_t lds = ((size_t)KT * (CL + D) + 4 * DMAX + ((nlist + 3) & ~3) + 4 * KMAX) * sizeof(float);   // <= 43 KiB
  if (KT == 2)
    rows_bwd_kernel<2><<<nblk, 256, lds, st>>>(Z, H, A_raw, stats, N, D, K, RB, Wc, dM, rv, lrow, lvec, nlist, dZ, dH,
                                               dwc_part, dbc_part);
  else if (KT == 4)
    rows_bwd_kernel<4><<<nblk, 256, lds, st>>>(Z, H, A_raw, stats, N, D, K, RB, Wc, dM, rv, lrow, lvec, nlist, dZ, dH,
                                               dwc_part, dbc_part);
  else
    rows_bwd_kernel<8><<<nblk, 256, lds, st>>>(Z, H, A_raw, stats, N, D, K, RB, Wc, dM, rv, lrow, lvec, nlist, dZ, dH,
                                               dwc_part, dbc_part);
  bwd_reduce_kernel<<<(K * D + K + 255) / 256, 256, 0, st>>>(dwc_part, dbc_part, nblk, K * D, K, dWc, dbc);
  TM_CHECK_LAUNCH();
  return 0;
}
