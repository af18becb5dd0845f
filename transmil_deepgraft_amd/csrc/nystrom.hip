// NystromAttention core (SURVEY.md section 8 App. A eq. 4-9), forward and backward.
//
// Replaces the arithmetic of the third-party `nystrom_attention.NystromAttention`
// called at code/models/TransMIL.py:26-34,47 (not vendored).
// Fixed geometry: dim_head = 64, num_landmarks = 256 (TransLayer always builds
// dim_head = dim/8, num_landmarks = dim/2 with dim = 512, code/models/TransMIL.py:26-31).
//
// Layouts in HBM (bh = bag*heads + head, n = n' = padded length, l = n/256):
//   q, k, v        [3][B*h][n][64]  T   (q pre-scaled by dim_head^-0.5)
//   ql, kl         [B*h][256][64]   fp32 (+ T copies for the MFMA paths)
//   merged out     [B][n][h*64]     T   (input of to_out)
//
// Forward (reassociated):  out = softmax(q kl^T) . (Z . (softmax(ql k^T) . v)) + conv33(v)
// i.e. attn1 @ (Z @ (attn3 @ v)) instead of (attn1 @ Z) @ (attn3 @ v): saves
// n*256*256*2 flop per head (8.86 GF/layer at N=8192); results agree to fp32
// rounding (tests/test_parity_gpu.py).
//
// One translation unit, one file per compute mode (T = float: parity, T = bf16: bench):
//   nystrom_common.h   geometry, LDS layouts, value fragments, BwdArgs: what both modes share
//   nystrom_f32.h      the parity kernels: a1_fwd, a3_fwd + a3_combine, conv_bwd, attn_bwd<MODE>
//   nystrom_bf16.h     the bench kernels: a1_fwd_bf16, a3_fwd_v2 + a3_combine_v2, conv_bwd_mfma,
//                      attn_bwd_bf16<MODE, NW, ST>, their diagnostic stamps and NysSel
// This file: the C entry points and launch helpers, and the kernels that serve both modes
//   landmarks        segment means of q, k (eq. 4)                 HBM-bound
//   sim2_softmax     A2 = softmax(ql kl^T) (eq. 5-6), fp32          tiny
//   softmax_bwd_rows dS2 = A2 * (dA2 - rowsum(dA2 * A2))
//   cast_rows        T copy of an fp32 matrix
//   assemble_dqkv    dq, dk, dv + landmark terms -> [B][n][3*h*64]
//   assemble_q_slab  the q part of dqkv with the A3 backward's dq~ slab reduced in the launch
#include <algorithm>
#include "common.h"
#include "nystrom_common.h"
#include "../../include/transmil_hip.h"

namespace {

// ---------------------------------------------------------------------------
// landmarks: out[bh][j][d] = sum_{t<l} x[bh][j*l+t][d] / l ; grid (nbh, 32), block 256: thread
// (landmark 8 blockIdx.y + tid / 32, d octet (tid / 4) % 8, row quarter tid % 4) sums its quarter of
// the l rows with 8-wide loads (all of them in flight for l <= 36), then the 4 quarters meet by
// xor shuffles in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void landmarks_kernel(const T* __restrict__ q, const T* __restrict__ k, int n,
                                                        int l, float* __restrict__ ql, float* __restrict__ kl,
                                                        T* __restrict__ ql_t, T* __restrict__ kl_t) {
  const int bh = blockIdx.x, tid = threadIdx.x, tq = tid & 3, o = ((tid >> 2) & 7) * 8;
  const int j = blockIdx.y * 8 + (tid >> 5);
  const int per = (l + 3) / 4, t0 = tq * per, t1 = min(l, t0 + per);
  const T* qp = q + ((size_t)bh * n + (size_t)j * l) * DH + o;
  const T* kp = k + ((size_t)bh * n + (size_t)j * l) * DH + o;
  float sq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sk[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = t0; t < t1; t += 9) {
    vec8<T> a[9], b[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int tt = min(t + u, t1 - 1);
      a[u] = load8(qp + (size_t)tt * DH);
      b[u] = load8(kp + (size_t)tt * DH);
    }
#pragma unroll
    for (int u = 0; u < 9; ++u)
      if (t + u < t1)
#pragma unroll
        for (int e = 0; e < 8; ++e) { sq[e] += to_f(a[u][e]); sk[e] += to_f(b[u][e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sq[e] += __shfl_xor(sq[e], 1, 64); sk[e] += __shfl_xor(sk[e], 1, 64);
    sq[e] += __shfl_xor(sq[e], 2, 64); sk[e] += __shfl_xor(sk[e], 2, 64);
  }
  if (tq) return;
  const float inv_l = (float)l;
  const size_t oo = ((size_t)bh * NL + j) * DH + o;
  float vq[8], vk[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { vq[e] = sq[e] / inv_l; vk[e] = sk[e] / inv_l; }
  *(f32x4*)(ql + oo) = (f32x4){vq[0], vq[1], vq[2], vq[3]};
  *(f32x4*)(ql + oo + 4) = (f32x4){vq[4], vq[5], vq[6], vq[7]};
  *(f32x4*)(kl + oo) = (f32x4){vk[0], vk[1], vk[2], vk[3]};
  *(f32x4*)(kl + oo + 4) = (f32x4){vk[4], vk[5], vk[6], vk[7]};
  vec8<T> tq8, tk8;
#pragma unroll
  for (int e = 0; e < 8; ++e) { tq8[e] = from_f<T>(vq[e]); tk8[e] = from_f<T>(vk[e]); }
  store8<T>(ql_t + oo, tq8);
  store8<T>(kl_t + oo, tk8);
}

// ---------------------------------------------------------------------------
// A2 = softmax_j(ql_i . kl_j), fp32 FMA.  grid (nbh, 256 / S2_ROWS), block 256: S2_ROWS rows per
// block, thread = column j.  k~ of the head arrives by coalesced 16-B loads (every load in flight
// at once) and is transposed into LDS ([64][260] fp32: thread j reads column j, conflict-free);
// the q~ rows are LDS broadcasts.
// a2s (optional): the same values as bf16 hi / lo planes (hi = bf16(a), lo = bf16(a - hi); lo plane at
// a2s + nbh * 256 * 256), the operand format of the split pseudo-inverse chain (pinv_split.hip).
constexpr int S2_ROWS = 8;

// A2 rows by ONE wave each (shared by sim2_softmax_kernel and the fused A3 forward, so both write
// the same bits): the wave computes RW rows -- q~ rows qrow0, qrow0 + qstep, .. of `qs` ([rows][64]
// fp32 in LDS) against the head's k~ in LDS as a row image [256][64] fp32 whose row j keeps its 16-B
// chunk c at slot c ^ (j & 15) (kimg: filled by LDS-DMA, k2_stage_dma) -- lane l owning columns l,
// l + 64, l + 128, l + 192 and reading each 4-d chunk of a row as one conflict-free 16-B read.  The
// logits keep the sequential fmaf order over d; the row max and sum are in-wave reductions (no LDS
// partials, no barrier: the 256-thread-per-row form spent ~9.7k of the A3 forward's cycles in its
// three barriers and cross-wave exchanges).  Output row k at o0 + k ostep.
constexpr int S2_KIMG = NL * DH;   // floats of the k~ row image

// k~ of head bh (kl [nbh][256][64] fp32) into the swizzled row image kimg by LDS-DMA: 64 pieces of
// 1 KB (4 rows), `nwaves` waves; lane L of a piece writes row 4 piece + L / 16, slot L % 16, i.e.
// fetches the row's chunk (L % 16) ^ (row & 15).  Completion: the issuing waves' vmcnt + a barrier.
TM_DEV void k2_stage_dma(float* kimg, const float* __restrict__ kl, int bh, int wave, int nwaves, int lane) {
  typedef __attribute__((address_space(3))) void lds_t;
  typedef __attribute__((address_space(1))) void glb_t;
  const float* kb = kl + (size_t)bh * NL * DH;
  for (int piece = wave; piece < 64; piece += nwaves) {
    const int row = piece * 4 + (lane >> 4), slot = lane & 15;
    __builtin_amdgcn_global_load_lds((glb_t*)(kb + (size_t)row * DH + (slot ^ (row & 15)) * 4),
                                     (lds_t*)(kimg + piece * 256), 16, 0, 0);
  }
}

template <int RW>
TM_DEV void sim2_wave_rows(const float* kimg, const float* qs, int qrow0, int qstep, int lane, float* __restrict__ a2,
                           bf16* __restrict__ a2s, size_t o0, size_t ostep, size_t plane) {
  float s[RW][4];
#pragma unroll
  for (int k = 0; k < RW; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) s[k][i] = 0.f;
  const int sw = lane & 15;   // (lane + 64 i) & 15
#pragma unroll 4
  for (int c = 0; c < DH; c += 4) {
    float kv[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 t = *(const f32x4*)(kimg + (lane + 64 * i) * DH + (((c >> 2) ^ sw) << 2));
#pragma unroll
      for (int e = 0; e < 4; ++e) kv[i][e] = t[e];
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const f32x4 q4 = *(const f32x4*)(qs + (qrow0 + k * qstep) * DH + c);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[k][i] = fmaf(q4[e], kv[i][e], s[k][i]);
    }
  }
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const float m = wave_max_dpp(fmaxf(fmaxf(s[k][0], s[k][1]), fmaxf(s[k][2], s[k][3])));
#pragma unroll
    for (int i = 0; i < 4; ++i) s[k][i] = __expf(s[k][i] - m);
    const float tot = wave_sum_dpp((s[k][0] + s[k][1]) + (s[k][2] + s[k][3]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t o = o0 + (size_t)k * ostep + lane + 64 * i;
      const float v = s[k][i] / tot;
      a2[o] = v;
      if (a2s) {
        const bf16 hi = (bf16)v;
        a2s[o] = hi;
        a2s[o + plane] = (bf16)(v - (float)hi);
      }
    }
  }
}

__global__ __launch_bounds__(256) void sim2_softmax_kernel(const float* __restrict__ ql, const float* __restrict__ kl,
                                                           float* __restrict__ a2, bf16* __restrict__ a2s) {
  const int bh = blockIdx.x, i0 = blockIdx.y * S2_ROWS, j = threadIdx.x;
  // one LDS array (the k~ row image, then the q~ rows): a second __shared__ object beside an LDS-DMA
  // target can make hipcc drain the DMA early (cdna_hip_programming.md section 5, trap 4(a))
  __shared__ __attribute__((aligned(16))) float lds[S2_KIMG + S2_ROWS * DH];
  float* kimg = lds;
  float* qs = lds + S2_KIMG;
  const int w = j >> 6;
  k2_stage_dma(kimg, kl, bh, w, 4, j & 63);
  {
    static_assert(S2_ROWS * DH % 256 == 0, "sim2: q~ rows per thread");
    constexpr int QE = S2_ROWS * DH / 256;
    float qv[QE];
#pragma unroll
    for (int u = 0; u < QE; ++u) qv[u] = ql[((size_t)bh * NL + i0) * DH + u * 256 + j];
#pragma unroll
    for (int u = 0; u < QE; ++u) qs[u * 256 + j] = qv[u];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's k~ pieces landed
  __syncthreads();
  // wave w: rows i0 + w and i0 + w + 4
  sim2_wave_rows<S2_ROWS / 4>(kimg, qs, w, 4, j & 63, a2, a2s, ((size_t)bh * NL + i0 + w) * NL, (size_t)4 * NL,
                              (size_t)gridDim.x * NL * NL);
}

// dS2 = A2 * (dA2 - rowsum(dA2 * A2)); grid (nbh*256/4), block 256 (one wave per row)
__global__ void softmax_bwd_rows_kernel(const float* __restrict__ a, const float* __restrict__ da,
                                        float* __restrict__ ds, int rows) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const f32x4 av = *(const f32x4*)(a + (size_t)r * NL + lane * 4);
  const f32x4 dv = *(const f32x4*)(da + (size_t)r * NL + lane * 4);
  const float s = wave_sum(av[0] * dv[0] + av[1] * dv[1] + av[2] * dv[2] + av[3] * dv[3]);
  f32x4 o;
  o[0] = av[0] * (dv[0] - s); o[1] = av[1] * (dv[1] - s); o[2] = av[2] * (dv[2] - s); o[3] = av[3] * (dv[3] - s);
  *(f32x4*)(ds + (size_t)r * NL + lane * 4) = o;
}

// T copy of an fp32 [rows][64] matrix
template <typename T>
__global__ void cast_rows_kernel(const float* __restrict__ x, T* __restrict__ y, long long count) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i + 8 <= count) {
    store8<T>(y + i, cvt8<T>(x + i));
  } else {
    for (long long j = i; j < count; ++j) y[j] = from_f<T>(x[j]);
  }
}

// ---------------------------------------------------------------------------
// dqkv[bag][t][which*h*64 + head*64 + d]:
//   q: scale * (dq[t] + dql[t/l] / l);  k: dk[t] + dkl[t/l] / l;  v: dv[t]
template <typename T>
__global__ void assemble_dqkv_kernel(const float* __restrict__ dq, const float* __restrict__ dql,
                                     const float* __restrict__ dk, const float* __restrict__ dkl,
                                     const float* __restrict__ dv, int n, int l, int nh, float scale,
                                     T* __restrict__ dqkv) {
  // item = (t, 8 consecutive columns of the 3*nh*64-wide row) of bag blockIdx.y;
  // grid (ceil(n * 3*nh*8 / 256), nbags), block 256.
  const int inner = nh * DH, per_row = 3 * inner / 8;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)n * per_row) return;
  const int c = (int)(item % per_row) * 8;
  const int t = (int)(item / per_row), bag = blockIdx.y;
  const int which = c / inner, head = (c % inner) / DH, d = c % DH;
  const size_t bh = (size_t)bag * nh + head;
  const size_t row = (bh * n + t) * DH + d;
  const size_t lrow = (bh * NL + t / l) * DH + d;
  const float inv_l = 1.0f / (float)l;
  const float* src = which == 0 ? dq : which == 1 ? dk : dv;
  const float* lsrc = which == 0 ? dql : dkl;
  const f32x4 a0 = *(const f32x4*)(src + row), a1 = *(const f32x4*)(src + row + 4);
  f32x4 b0 = (f32x4){}, b1 = (f32x4){};
  if (which < 2) { b0 = *(const f32x4*)(lsrc + lrow); b1 = *(const f32x4*)(lsrc + lrow + 4); }
  const float a[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  const float b[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
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

// q part of dqkv with the A3 backward's dq~ partial slab reduced in the same launch (no separate
// split-K reduce, no dq~3 round trip): q = scale * (dq + (dql + sum_p slab[p])[t / l] / l).
// grid (256 landmarks, nbags), block 512: the workgroup's first QP dq pieces per thread are
// requested first, then landmark j's slab row is summed (eight part groups, combined in a fixed
// order) while they are in flight, then the l tokens of segment j are written.
// INPLACE (bf16): the q rows already hold bf16(scale * dq) (tm_nys_a1_bwd_dqkv); the landmark term
// scale * (dql + sum_p slab[p])[t / l] / l is added to them in place.
constexpr int AQ_THREADS = 512, AQ_GROUPS = AQ_THREADS / 64, AQ_QP = 5;
template <typename T, bool INPLACE = false>
__global__ __launch_bounds__(AQ_THREADS) void assemble_q_slab_kernel(const float* __restrict__ dq, int dq_row,
                                                                     const float* __restrict__ dql,
                                                                     const bf16* __restrict__ slab, int slabs,
                                                                     long long slab_count, int n, int l, int nh,
                                                                     float scale, T* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) float part[AQ_GROUPS][8 * DH];   // [group][nh <= 8 heads x 64 d]
  const int j = blockIdx.x, bag = blockIdx.y, tid = threadIdx.x;
  const int inner = nh * DH, pieces = inner / 8;                          // <= 64
  const int items = l * pieces;
  auto dq_row_of = [&](int it, int& t, int& c) -> size_t {
    t = j * l + it / pieces;
    c = (it % pieces) * 8;
    return (((size_t)bag * nh + c / DH) * n + t) * DH + c % DH;
  };
  auto load_q = [&](int it) -> f32x8 {
    int t, c;
    const size_t row = dq_row_of(it, t, c);
    if constexpr (INPLACE) {
      const vec8<T> v = load8<T>(dqkv + ((size_t)bag * n + t) * (3 * inner) + c);
      f32x8 r;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = to_f(v[e]);
      return r;
    } else {
      return (dq_row < 0 || t == dq_row) ? load8<float>(dq + row) : (f32x8){};
    }
  };
  f32x8 a[AQ_QP];
#pragma unroll
  for (int u = 0; u < AQ_QP; ++u) {
    const int it = tid + AQ_THREADS * u;
    a[u] = it < items ? load_q(it) : (f32x8){};
  }
  {
    const int pc = tid & 63, g = tid >> 6;
    if (pc < pieces) {
      const int c = pc * 8, head = c / DH, d = c % DH;
      const size_t off = (((size_t)bag * nh + head) * NL + j) * DH + d;
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      int p = g;
      for (; p + 3 * AQ_GROUPS < slabs; p += 4 * AQ_GROUPS) {   // four partials in flight per thread
        bf16x8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = load8<bf16>(slab + (size_t)(p + AQ_GROUPS * u) * slab_count + off);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += (float)v[u][e];
      }
      for (; p < slabs; p += AQ_GROUPS) {
        const bf16x8 v = load8<bf16>(slab + (size_t)p * slab_count + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) part[g][c + e] = acc[e];
    }
  }
  __syncthreads();
  for (int col = tid; col < inner; col += AQ_THREADS) {   // pairwise over the groups, then the landmark path's dq~
    const int head = col / DH, d = col % DH;
    const float sum = ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) +
                      ((part[4][col] + part[5][col]) + (part[6][col] + part[7][col]));
    part[0][col] = (dql[(((size_t)bag * nh + head) * NL + j) * DH + d] + sum) * (1.0f / (float)l);
  }
  __syncthreads();
  auto store = [&](int it, const f32x8& av) {
    int t, c;
    (void)dq_row_of(it, t, c);
    vec8<T> out;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      out[e] = INPLACE ? from_f<T>(av[e] + scale * part[0][c + e]) : from_f<T>(scale * (av[e] + part[0][c + e]));
    store8<T>(dqkv + ((size_t)bag * n + t) * (3 * inner) + c, out);
  };
#pragma unroll
  for (int u = 0; u < AQ_QP; ++u)
    if (tid + AQ_THREADS * u < items) store(tid + AQ_THREADS * u, a[u]);
  for (int it = tid + AQ_THREADS * AQ_QP; it < items; it += AQ_THREADS)   // long segments (l > 40)
    store(it, load_q(it));
}

}  // namespace

// the two pipelines (nystrom_bf16.h after the kernels above: its A3 forward calls sim2_wave_rows)
#include "nystrom_f32.h"
#include "nystrom_bf16.h"

// gemm.hip (library-internal): split-K sum of fp32 or bf16 partial slabs, deferred into q when given
int tm_splitk_reduce_typed(const void* slab, int slab_dtype, float* out, int splits, long long count, float alpha,
                           int accumulate, tm_reduce_queue* q, void* stream);

// ============================ C entry points ===============================
#ifdef TM_DIAG
extern "C" void tm_debug_set_nys_sel(int sel) { g_nys_sel = sel; }   // a NysSel
// copy the stamped kernels' stamps ([block][wave][8] u64) to a host buffer (diagnostics only)
extern "C" int tm_debug_a1_stamps(unsigned long long* host, int count) {
  TM_REQUIRE(count > 0 && count <= 512 * 8 * 8, "a1_stamps: bad count");
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_a1_stamps), count * sizeof(unsigned long long)) != hipSuccess) {
    tm_set_error("a1_stamps: copy");
    return 2;
  }
  return 0;
}
#endif

// The kernels that serve both modes are instantiated per dtype (TM_DTYPE_DISPATCH); where the
// modes have kernels of their own, the entry point takes its TM_BF16 branch first and the rest
// must be TM_F32 (TM_REQUIRE_F32).
#define TM_BAD_DTYPE "nystrom: dtype must be TM_F32 or TM_BF16"
#define TM_DTYPE_DISPATCH(dt, CALL)                               \
  if ((dt) == TM_BF16) { using T = bf16; CALL; }                  \
  else if ((dt) == TM_F32) { using T = float; CALL; }             \
  else { tm_set_error(TM_BAD_DTYPE); return 1; }
#define TM_REQUIRE_F32(dt) TM_REQUIRE((dt) == TM_F32, TM_BAD_DTYPE)

extern "C" int tm_nys_landmarks(int dtype, const void* q, const void* k, int nbh, int n, float* ql, float* kl,
                                void* ql_t, void* kl_t, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0, "landmarks: n must be a positive multiple of 256");
  const int l = n / NL;
  TM_DTYPE_DISPATCH(dtype, (landmarks_kernel<T><<<dim3(nbh, NL / 8), 256, 0, (hipStream_t)stream>>>(
                               (const T*)q, (const T*)k, n, l, ql, kl, (T*)ql_t, (T*)kl_t)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_sim2_softmax(const float* ql, const float* kl, int nbh, float* a2, void* stream) {
  sim2_softmax_kernel<<<dim3(nbh, NL / S2_ROWS), 256, 0, (hipStream_t)stream>>>(ql, kl, a2, nullptr);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_sim2_softmax_split(const float* ql, const float* kl, int nbh, float* a2, void* a2s,
                                         void* stream) {
  TM_REQUIRE(a2s, "sim2_softmax_split: a2s is required");
  sim2_softmax_kernel<<<dim3(nbh, NL / S2_ROWS), 256, 0, (hipStream_t)stream>>>(ql, kl, a2, (bf16*)a2s);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_softmax_bwd_rows256(const float* a, const float* da, float* ds, int rows, void* stream) {
  softmax_bwd_rows_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(a, da, ds, rows);
  TM_CHECK_LAUNCH();
  return 0;
}

// key splits (partials per head) of the bf16 A3 forward
extern "C" long long tm_nys_a3_partials(int nbh, int n) { return a3v_splits(nbh, n); }

extern "C" long long tm_nys_a3_workspace(int nbh, int n) {
  const long long parts = std::max((long long)(n / NL), (long long)a3v_splits(nbh, n));
  return parts * nbh * NL * (DH + 2) * (long long)sizeof(float);
}

namespace {
// the bf16 key-split launch (+ the fused A2 rows when s2.a2 is set and the split allows it)
void launch_a3_fwd_v2(const float* ql, const void* k, const void* v, int nbh, int n, float* work, Sim2Out s2,
                      hipStream_t st) {
  const int P = a3v_splits(nbh, n);
  bf16* po = (bf16*)work;                          // bf16 partial sums in the first half of an fp32-sized region
  float* pm = work + (size_t)P * nbh * NL * DH;
  float* pl = pm + (size_t)P * nbh * NL;
  const dim3 grid(P, nbh);
  const bf16* kb = (const bf16*)k;
  const bf16* vb = (const bf16*)v;
#ifdef TM_DIAG
  if (NYS_SEL == NYS_STAMP_A3_FWD && !s2.a2) {   // s_memtime stamps per wave (tm_debug_a1_stamps)
    tm_allow_smem(a3_fwd_v2_kernel<1>, A3V_BYTES);
    a3_fwd_v2_kernel<1><<<grid, 512, A3V_BYTES, st>>>(ql, kb, vb, n, P, po, pm, pl, s2);
    return;
  }
  if (NYS_SEL == NYS_STAMP_A3_FWD && s2.a2 && P * 8 == NL) {   // the same with the fused A2 rows
    tm_allow_smem(a3_fwd_v2_kernel<1, 4>, A3V_BYTES);
    a3_fwd_v2_kernel<1, 4><<<grid, 512, A3V_BYTES, st>>>(ql, kb, vb, n, P, po, pm, pl, s2);
    return;
  }
#endif
  if (s2.a2 && P * 8 == NL) {
    tm_allow_smem(a3_fwd_v2_kernel<0, 4>, A3V_BYTES);
    a3_fwd_v2_kernel<0, 4><<<grid, 512, A3V_BYTES, st>>>(ql, kb, vb, n, P, po, pm, pl, s2);
  } else if (s2.a2 && P * 16 == NL) {
    tm_allow_smem(a3_fwd_v2_kernel<0, 8>, A3V_BYTES);
    a3_fwd_v2_kernel<0, 8><<<grid, 512, A3V_BYTES, st>>>(ql, kb, vb, n, P, po, pm, pl, s2);
  } else {
    tm_allow_smem(a3_fwd_v2_kernel<0>, A3V_BYTES);
    a3_fwd_v2_kernel<0><<<grid, 512, A3V_BYTES, st>>>(ql, kb, vb, n, P, po, pm, pl, s2);
    if (s2.a2)   // a split the fused rows do not tile: the separate launch
      sim2_softmax_kernel<<<dim3(nbh, NL / S2_ROWS), 256, 0, st>>>(ql, s2.kl, s2.a2, s2.a2s);
  }
}
}  // namespace

extern "C" int tm_nys_a3_fwd(int dtype, const float* ql, const void* k, const void* v, int nbh, int n, float* work,
                             float* w, float* lse3, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0, "a3_fwd: n must be a positive multiple of 256");
  TM_REQUIRE((w && lse3) || dtype == TM_BF16, "a3_fwd: w / lse3 may be null (deferred combine) in bf16 mode only");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) {
    launch_a3_fwd_v2(ql, k, v, nbh, n, work, Sim2Out{nullptr, nullptr, nullptr}, st);
    TM_CHECK_LAUNCH();
    if (!w) return 0;   // deferred: the combine runs in the pseudo-inverse chain (tm_pinv_fwd_split_a3)
    const int P = a3v_splits(nbh, n);
    const bf16* po = (const bf16*)work;
    float* pm = work + (size_t)P * nbh * NL * DH;
    float* pl = pm + (size_t)P * nbh * NL;
    a3_combine_v2_kernel<<<dim3(nbh, NL / 8), 256, 0, st>>>(A3Combine{po, pm, pl, P, nbh, w, lse3});
    TM_CHECK_LAUNCH();
    return 0;
  }
  TM_REQUIRE_F32(dtype);
  const int nkb = n / NL;
  float* po = work;
  float* pm = po + (size_t)nkb * nbh * NL * DH;
  float* pl = pm + (size_t)nkb * nbh * NL;
  tm_allow_smem(a3_fwd_kernel, FWD_F32_SMEM);
  a3_fwd_kernel<<<dim3(nkb, nbh, 2), 256, FWD_F32_SMEM, st>>>(ql, (const float*)k, (const float*)v, n, po, pm, pl);
  TM_CHECK_LAUNCH();
  a3_combine_kernel<<<dim3(nbh, NL / 16), 256, 0, st>>>(po, pm, pl, nkb, nbh, w, lse3);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_a3_fwd_sim2(const float* ql, const float* kl, const void* k, const void* v, int nbh, int n,
                                  float* work, float* a2, void* a2s, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0, "a3_fwd_sim2: n must be a positive multiple of 256");
  TM_REQUIRE(ql && kl && k && v && work && a2 && a2s, "a3_fwd_sim2: null operand");
  launch_a3_fwd_v2(ql, k, v, nbh, n, work, Sim2Out{kl, a2, (bf16*)a2s}, (hipStream_t)stream);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_a1_fwd(int dtype, const void* q, const void* v, const void* kl_t, const void* y_t,
                             const float* wconv, int nbh, int nh, int n, void* merged, float* lse1, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0 && nbh % nh == 0, "a1_fwd: bad shape");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) {
    const int cph = n / 32;
    int wpg = std::max(1, std::min(tm_cu_count() / std::max(nbh, 1), cph));
    wpg = std::max(wpg, (cph + A1P_MAXCH - 1) / A1P_MAXCH);  // <= A1P_MAXCH chunks per workgroup
    auto kern = a1_fwd_bf16_kernel<false>;
#ifdef TM_DIAG
    if (NYS_SEL == NYS_STAMP_A1_FWD) kern = a1_fwd_bf16_kernel<true>;
#endif
    tm_allow_smem(kern, A1P_BYTES);
    kern<<<dim3(wpg, nbh), 256, A1P_BYTES, st>>>((const bf16*)q, (const bf16*)v, (const bf16*)kl_t,
                                                               (const bf16*)y_t, wconv, n, nh, wpg, (bf16*)merged,
                                                               lse1);
    TM_CHECK_LAUNCH();
    return 0;
  }
  TM_REQUIRE_F32(dtype);
  constexpr size_t sm = FWD_F32_SMEM > A1_EPI_BYTES ? FWD_F32_SMEM : A1_EPI_BYTES;
  tm_allow_smem(a1_fwd_kernel, sm);
  a1_fwd_kernel<<<dim3(n / 128, nbh), 256, sm, st>>>((const float*)q, (const float*)v, (const float*)kl_t,
                                                     (const float*)y_t, wconv, n, nh, (float*)merged, lse1);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_cast_f32(int dtype, const float* x, void* y, long long count, void* stream) {
  if (count == 0) return 0;
  TM_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "cast_f32: 16-B aligned buffers");
  TM_DTYPE_DISPATCH(dtype, (cast_rows_kernel<T><<<(unsigned)((count + 2047) / 2048), 256, 0, (hipStream_t)stream>>>(
                               x, (T*)y, count)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_nys_conv_bwd_workspace(int nbags, int nh, int n) {
  const int r = conv_bwd_rows(nbags * nh, n);
  const long long blocks = std::max((n + 63) / 64, (n + r - 1) / r);
  return (long long)nbags * blocks * nh * TAPS * (long long)sizeof(float);
}

extern "C" int tm_nys_conv_bwd(int dtype, const void* dmerged, const void* merged, const void* v, const float* wconv,
                               int nbh, int nh, int n, void* dv, float* d1, float* work, float* dwconv,
                               tm_reduce_queue* rq, void* stream) {
  TM_REQUIRE(nbh % nh == 0 && n > 0, "conv_bwd: bad shape");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) {
    const int r = conv_bwd_rows(nbh, n), nblk = (n + r - 1) / r;
    tm_allow_smem(conv_bwd_mfma_kernel, CbLay::BYTES);
    conv_bwd_mfma_kernel<<<dim3(nblk, nbh), 512, CbLay::BYTES, st>>>(
        (const bf16*)dmerged, (const bf16*)merged, (const bf16*)v, wconv, n, nh, r, (bf16*)dv, d1, work);
    TM_CHECK_LAUNCH();
    return tm_splitk_reduce(work, dwconv, (nbh / nh) * nblk, (long long)nh * TAPS, 1.0f, 0, rq, stream);
  }
  TM_REQUIRE_F32(dtype);
  const int ntb = (n + 63) / 64;
  conv_bwd_kernel<<<dim3(ntb, nbh), 256, 0, st>>>((const float*)dmerged, (const float*)merged, (const float*)v, wconv,
                                                  n, nh, (float*)dv, d1, work);
  TM_CHECK_LAUNCH();
  return tm_splitk_reduce(work, dwconv, (nbh / nh) * ntb, (long long)nh * TAPS, 1.0f, 0, rq, stream);
}

// A1 backward: keys = landmarks kl_t [bh][256][64], values = y_t, queries = q rows, dO = dmerged.
// dq (fp32 [bh][n][64]) written; dkl/dy partial slabs [n/qpw][bh][256][64] in work.
namespace {
// workgroups per head of the bf16 A1 backward (even split of the n / 32 query chunks)
int a1_bwd_split(int nbh, int n) {
  const int cph = n / 32;
  const int w = std::min(cph, std::max(1, tm_cu_count() / std::max(nbh, 1)));
  return std::max(w, (cph + BwdLay16::MAXQ / 32 - 1) / (BwdLay16::MAXQ / 32));
}
}  // namespace

extern "C" long long tm_nys_a1_bwd_workspace(int nbh, int n, int queries_per_wg) {
  const long long slabs = std::max((long long)(n / queries_per_wg), (long long)a1_bwd_split(nbh, n));
  return 2LL * slabs * nbh * NL * DH * (long long)sizeof(float);
}

namespace {
int a1_bwd_impl(int dtype, const void* q, const void* dmerged, const void* kl_t, const void* y_t, const float* lse1,
                const float* d1, int nbh, int nh, int n, int queries_per_wg, float* dq, void* dqkv, float dq_scale,
                float* work, float* dkl, float* dy, int accumulate, tm_reduce_queue* rq, void* stream);
}  // namespace

extern "C" int tm_nys_a1_bwd(int dtype, const void* q, const void* dmerged, const void* kl_t, const void* y_t,
                             const float* lse1, const float* d1, int nbh, int nh, int n, int queries_per_wg,
                             float* dq, float* work, float* dkl, float* dy, int accumulate, tm_reduce_queue* rq,
                             void* stream) {
  return a1_bwd_impl(dtype, q, dmerged, kl_t, y_t, lse1, d1, nbh, nh, n, queries_per_wg, dq, nullptr, 0.f, work, dkl,
                     dy, accumulate, rq, stream);
}

// bf16 only: dq goes to the q part of dqkv as bf16(dq_scale * dq) (tm_nys_assemble_q_slab_inplace
// then adds the landmark term in place)
extern "C" int tm_nys_a1_bwd_dqkv(const void* q, const void* dmerged, const void* kl_t, const void* y_t,
                                  const float* lse1, const float* d1, int nbh, int nh, int n, void* dqkv,
                                  float dq_scale, float* work, float* dkl, float* dy, tm_reduce_queue* rq,
                                  void* stream) {
  TM_REQUIRE(dqkv && ((uintptr_t)dqkv % 16) == 0 && nbh % nh == 0, "a1_bwd_dqkv: dqkv");
  return a1_bwd_impl(TM_BF16, q, dmerged, kl_t, y_t, lse1, d1, nbh, nh, n, 256, nullptr, dqkv, dq_scale, work, dkl,
                     dy, 0, rq, stream);
}

namespace {
int a1_bwd_impl(int dtype, const void* q, const void* dmerged, const void* kl_t, const void* y_t, const float* lse1,
                const float* d1, int nbh, int nh, int n, int queries_per_wg, float* dq, void* dqkv, float dq_scale,
                float* work, float* dkl, float* dy, int accumulate, tm_reduce_queue* rq, void* stream) {
  TM_REQUIRE(queries_per_wg % 32 == 0 && n % queries_per_wg == 0, "a1_bwd: queries_per_wg must divide n, x32");
  TM_REQUIRE(dtype != TM_BF16 || queries_per_wg <= NL, "a1_bwd: queries_per_wg must be <= 256 in bf16 mode");
  const bool split = dtype == TM_BF16;
  TM_REQUIRE(!dqkv || split, "a1_bwd_dqkv: the bf16 split kernel only");
  const int nqc = split ? a1_bwd_split(nbh, n) : n / queries_per_wg;
  BwdArgs a{};
  a.q = q; a.q_bag = (long long)nh * n * DH; a.q_head = (long long)n * DH; a.q_row = DH;
  a.dO = dmerged; a.o_bag = (long long)n * nh * DH; a.o_head = DH; a.o_row = nh * DH;
  a.k = kl_t; a.k_bag = (long long)nh * NL * DH; a.k_head = (long long)NL * DH;
  a.v = y_t; a.v_bag = a.k_bag; a.v_head = a.k_head;
  a.lse = lse1; a.lse_bh = n; a.dd = d1; a.dd_bh = n;
  a.dq = dq; a.dq_bh = (long long)n * DH;
  a.dqkv = dqkv; a.dq_scale = dq_scale;
  float* slab_k = work;
  float* slab_v = work + (size_t)nqc * nbh * NL * DH;
  a.dk = slab_k; a.dk_bh = (long long)NL * DH;
  a.dv = slab_v; a.dv_bh = (long long)NL * DH;
  a.slab_stride = (long long)nbh * NL * DH;
  a.nh = nh; a.n_queries_per_wg = queries_per_wg; a.n_key_rows = NL;
  hipStream_t st = (hipStream_t)stream;
  if (split) {
    a.q_total = n;
    a.slab_bf16 = 1;   // the dk~ / dY partials as bf16
    auto kern = attn_bwd_bf16_kernel<MODE_A1>;
#ifdef TM_DIAG
    if (NYS_SEL == NYS_STAMP_A1_BWD) kern = attn_bwd_bf16_kernel<MODE_A1, 8, 1>;
    if (NYS_SEL == NYS_STAMP_A1_BWD_CHUNK) kern = attn_bwd_bf16_kernel<MODE_A1, 8, 2>;
#endif
    tm_allow_smem(kern, BwdLay16::BYTES);
    kern<<<dim3(nqc, nbh), 512, BwdLay16::BYTES, st>>>(a);
  } else {
    TM_REQUIRE_F32(dtype);
    tm_allow_smem(attn_bwd_kernel<MODE_A1>, BwdLayF32::BYTES);
    attn_bwd_kernel<MODE_A1><<<dim3(nqc, nbh), 512, BwdLayF32::BYTES, st>>>(a);
  }
  TM_CHECK_LAUNCH();
  const long long cnt = (long long)nbh * NL * DH;
  const int sdt = a.slab_bf16 ? TM_BF16 : TM_F32;
  int rc = tm_splitk_reduce_typed(slab_k, sdt, dkl, nqc, cnt, 1.0f, accumulate, rq, stream);
  if (rc) return rc;
  return tm_splitk_reduce_typed(slab_v, sdt, dy, nqc, cnt, 1.0f, 0, rq, stream);
}
}  // namespace

// A3 backward: keys = k rows, values = v rows, queries = ql_t (256 landmarks), dO = dw_t.
// dk written (=), dv accumulated (+=), dql accumulated from partial slabs.
namespace {
// bf16 A3 backward grid: the head's n / 32 key units split evenly over 256 / nbh workgroups when
// that is <= 9 units each (one chip round; the 9-wave form), else over ceil(units / 8) workgroups
// of the 8-wave form.  Every workgroup writes one dq~ partial slab.
struct A3Split { int wpg, nw; };
A3Split a3_bwd_split(int nbh, int n) {
  const int units = n / 32;
  const int w = std::max(1, std::min(units, tm_cu_count() / std::max(nbh, 1)));
  const int per = (units + w - 1) / w;
  if (per <= 8) return {w, 8};
  if (per == 9) return {w, 9};
  return {(units + 7) / 8, 8};
}

void launch_a3_bwd_bf16(BwdArgs& a, int nbh, int n, hipStream_t st, int& slabs) {
  const A3Split sp = a3_bwd_split(nbh, n);
  a.q_total = n;  // even split on
  slabs = sp.wpg;
  if (sp.nw == 9) {
    auto kern = attn_bwd_bf16_kernel<MODE_A3, 9>;
#ifdef TM_DIAG
    if (NYS_SEL == NYS_STAMP_A3_BWD) kern = attn_bwd_bf16_kernel<MODE_A3, 9, 1>;
    if (NYS_SEL == NYS_STAMP_A3_BWD_CHUNK) kern = attn_bwd_bf16_kernel<MODE_A3, 9, 2>;
#endif
    tm_allow_smem(kern, BwdLay9::BYTES);
    kern<<<dim3(sp.wpg, nbh), 576, BwdLay9::BYTES, st>>>(a);
  } else {
    tm_allow_smem(attn_bwd_bf16_kernel<MODE_A3, 8>, BwdLay16::BYTES);
    attn_bwd_bf16_kernel<MODE_A3, 8><<<dim3(sp.wpg, nbh), 512, BwdLay16::BYTES, st>>>(a);
  }
}
}  // namespace

extern "C" long long tm_nys_a3_bwd_workspace(int nbh, int n) {
  const long long slabs = std::max((long long)(n / NL), (long long)a3_bwd_split(nbh, n).wpg);
  return slabs * nbh * NL * DH * (long long)sizeof(float);
}

extern "C" int tm_nys_a3_bwd(int dtype, const void* ql_t, const void* dw_t, const void* k, const void* v,
                             const float* lse3, const float* d3, int nbh, int nh, int n, float* dk, float* dv,
                             float* work, float* dql, int accumulate, tm_reduce_queue* rq, void* stream) {
  TM_REQUIRE(n % NL == 0, "a3_bwd: n must be a multiple of 256");
  const int nkb = n / NL;
  BwdArgs a{};
  a.q = ql_t; a.q_bag = (long long)nh * NL * DH; a.q_head = (long long)NL * DH; a.q_row = DH;
  a.dO = dw_t; a.o_bag = a.q_bag; a.o_head = a.q_head; a.o_row = DH;
  a.k = k; a.k_bag = (long long)nh * n * DH; a.k_head = (long long)n * DH;
  a.v = v; a.v_bag = a.k_bag; a.v_head = a.k_head;
  a.lse = lse3; a.lse_bh = NL; a.dd = d3; a.dd2 = d3 + (size_t)nbh * NL; a.dd_bh = NL;   // [2][nbh][256] partials
  a.dq = work; a.dq_bh = (long long)NL * DH;
  a.slab_stride = (long long)nbh * NL * DH;
  a.dk = dk; a.dk_bh = (long long)n * DH;
  a.dv = dv; a.dv_bh = (long long)n * DH;
  a.nh = nh; a.n_queries_per_wg = NL; a.n_key_rows = n;
  hipStream_t st = (hipStream_t)stream;
  int slabs = nkb;
  if (dtype == TM_BF16) {
    launch_a3_bwd_bf16(a, nbh, n, st, slabs);
  } else {
    TM_REQUIRE_F32(dtype);
    tm_allow_smem(attn_bwd_kernel<MODE_A3>, BwdLayF32::BYTES);
    attn_bwd_kernel<MODE_A3><<<dim3(nkb, nbh), 512, BwdLayF32::BYTES, st>>>(a);
  }
  TM_CHECK_LAUNCH();
  return tm_splitk_reduce(work, dql, slabs, (long long)nbh * NL * DH, 1.0f, accumulate, rq, stream);
}

// bf16 A3 backward with the fused key-side epilogue: the final k / v parts of dqkv from dK, dV,
// the conv backward's dv (fp32, read) and dk~ (fp32 [bh][256][64], after the pseudo-inverse
// backward); dql3 (=) from the per-key-block slabs.
extern "C" int tm_nys_a3_bwd_fused(const void* ql_t, const void* dw_t, const void* k, const void* v,
                                   const float* lse3, const float* d3, int nbh, int nh, int n, const void* dv_conv,
                                   int dv_lo, int dv_hi, const float* dkl, float* work, float* dql, void* dqkv,
                                   tm_reduce_queue* rq, void* stream) {
  TM_REQUIRE(n % NL == 0 && nbh % nh == 0, "a3_bwd_fused: n must be a multiple of 256");
  TM_REQUIRE(dv_conv && dkl && dqkv, "a3_bwd_fused: null operand");
  const int nkb = n / NL;
  BwdArgs a{};
  a.q = ql_t; a.q_bag = (long long)nh * NL * DH; a.q_head = (long long)NL * DH; a.q_row = DH;
  a.dO = dw_t; a.o_bag = a.q_bag; a.o_head = a.q_head; a.o_row = DH;
  a.k = k; a.k_bag = (long long)nh * n * DH; a.k_head = (long long)n * DH;
  a.v = v; a.v_bag = a.k_bag; a.v_head = a.k_head;
  a.lse = lse3; a.lse_bh = NL; a.dd = d3; a.dd2 = d3 + (size_t)nbh * NL; a.dd_bh = NL;   // [2][nbh][256] partials
  a.dq = work; a.dq_bh = (long long)NL * DH;
  a.slab_stride = (long long)nbh * NL * DH;
  a.dv = (float*)dv_conv; a.dv_bh = (long long)n * DH;   // bf16 rows (the kernel reads them as bf16)
  a.nh = nh; a.n_queries_per_wg = NL; a.n_key_rows = n;
  a.dqkv = dqkv; a.dkl = dkl; a.l = n / NL; a.inv_l = 1.0f / (float)(n / NL);
  a.dv_lo = dv_lo; a.dv_hi = dv_hi;
  hipStream_t st = (hipStream_t)stream;
  int slabs = nkb;
  a.slab_bf16 = 1;      // the dq~ partials as bf16 ([slabs][B*h][256][64], summed in fp32 by the consumer)
  launch_a3_bwd_bf16(a, nbh, n, st, slabs);
  TM_CHECK_LAUNCH();
  if (!dql) return 0;   // the slab stays for tm_nys_assemble_q_slab
  return tm_splitk_reduce_typed(work, TM_BF16, dql, slabs, (long long)nbh * NL * DH, 1.0f, 0, rq, stream);
}

extern "C" int tm_nys_a3_bwd_slabs(int nbh, int n) { return a3_bwd_split(nbh, n).wpg; }

extern "C" int tm_nys_assemble_q_slab(int dtype, const float* dq, int dq_row, const float* dql, const void* slab,
                                      int slabs, int nbags, int nh, int n, float scale, void* dqkv, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0 && nh > 0 && nh <= 8 && slabs > 0, "assemble_q_slab: bad shape");
  TM_REQUIRE(dq && dql && slab && dqkv, "assemble_q_slab: null operand");
  TM_DTYPE_DISPATCH(dtype, (assemble_q_slab_kernel<T><<<dim3(NL, nbags), AQ_THREADS, 0, (hipStream_t)stream>>>(
                               dq, dq_row, dql, (const bf16*)slab, slabs, (long long)nbags * nh * NL * DH, n, n / NL,
                               nh, scale, (T*)dqkv)));
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_assemble_q_slab_inplace(const float* dql, const void* slab, int slabs, int nbags, int nh, int n,
                                              float scale, void* dqkv, void* stream) {
  TM_REQUIRE(n > 0 && n % NL == 0 && nh > 0 && nh <= 8 && slabs > 0, "assemble_q_slab_inplace: bad shape");
  TM_REQUIRE(dql && slab && dqkv && ((uintptr_t)dqkv % 16) == 0, "assemble_q_slab_inplace: null / misaligned operand");
  assemble_q_slab_kernel<bf16, true><<<dim3(NL, nbags), AQ_THREADS, 0, (hipStream_t)stream>>>(
      nullptr, -1, dql, (const bf16*)slab, slabs, (long long)nbags * nh * NL * DH, n, n / NL, nh, scale, (bf16*)dqkv);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" int tm_nys_assemble_dqkv(int dtype, const float* dq, const float* dql, const float* dk, const float* dkl,
                                    const float* dv, int nbags, int nh, int n, float scale, void* dqkv,
                                    void* stream) {
  TM_REQUIRE(n % NL == 0, "assemble_dqkv: n must be a multiple of 256");
  const long long items = (long long)n * 3 * nh * DH / 8;
  TM_DTYPE_DISPATCH(dtype, (assemble_dqkv_kernel<T><<<dim3((unsigned)((items + 255) / 256), nbags), 256, 0,
                                                       (hipStream_t)stream>>>(
                               dq, dql, dk, dkl, dv, n, n / NL, nh, scale, (T*)dqkv)));
  TM_CHECK_LAUNCH();
  return 0;
}
