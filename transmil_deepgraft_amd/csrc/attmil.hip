// AttMIL gated attention pooling (code/models/AttMIL.py:88-110), fp32, the non-GEMM half:
//   a_i   = w . (tanh(Zv_i) * sigmoid(Zu_i)) + b        Z = H [Wv;Wu]^T + [bv;bu] (the caller's GEMM)
//   p     = softmax_N(a)                                 (:101-104)
//   M     = sum_i p_i H_i ;  logits = M Wc^T + bc         (:105-106)
// and its backward down to dZ (the caller's GEMMs take dZ to dH, d[Wv;Wu], d[bv;bu]):
//   dM = dl Wc ; dWc = dl^T M ; dbc = dl
//   dp_i = H_i . dM ; da_i = p_i (dp_i - sum_j p_j dp_j)
//   dZv = da w sig (1 - tanh^2) ; dZu = da w tanh sig (1 - sig) ; dw = sum_i da tanh sig ; db = sum_i da
//   dH_i = p_i dM   (the GEMM then adds dZ [Wv;Wu])
// HBM-bound row passes over H [N, L] and Z [N, 2D]; every reduction is a fixed-order tree, so
// results are deterministic run to run.
#include "common.h"
#include "mil_common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int POOL_ROWS = 64;     // rows of H per pooling / backward-row block

// one wave per instance row: a_i = sum_d tanh(Z[i][d]) sigmoid(Z[i][D+d]) w[d] + b
__global__ void __launch_bounds__(256) score_kernel(const float* __restrict__ Z, int N, int D,
                                                    const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const float* z = Z + (size_t)i * 2 * D;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) acc += tanhf(z[d]) * sigmoid_fast(z[D + d]) * w[d];
  acc = wave_sum(acc);
  if (lane == 0) a[i] = acc + b[0];
}

// softmax statistics over all N scores: stats = {max, sum exp(a - max)}; one block
__global__ void __launch_bounds__(1024) stats_kernel(const float* __restrict__ a, int N, float* __restrict__ stats) {
  __shared__ float red[16];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < N; i += blockDim.x) m = fmaxf(m, a[i]);
  m = block_reduce<true>(m, red);
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += blockDim.x) s += __expf(a[i] - m);
  s = block_reduce<false>(s, red);
  if (threadIdx.x == 0) {
    stats[0] = m;
    stats[1] = s;
  }
}

// partial[blk][c] = sum over this block's rows of p_i H[i][c]; also p_i; block = L/4 threads (float4 columns)
__global__ void pool_partial_kernel(const float* __restrict__ a, const float* __restrict__ stats,
                                    const float* __restrict__ H, int N, int L, float* __restrict__ p,
                                    float* __restrict__ partial) {
  const int r0 = blockIdx.x * POOL_ROWS, r1 = min(N, r0 + POOL_ROWS), t = threadIdx.x;
  const float m = stats[0], inv = 1.f / stats[1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = r0; i < r1; ++i) {
    const float pi = __expf(a[i] - m) * inv;
    if (t == 0) p[i] = pi;
    const f32x4 h = *(const f32x4*)(H + (size_t)i * L + 4 * t);
    acc += pi * h;
  }
  *(f32x4*)(partial + (size_t)blockIdx.x * L + 4 * t) = acc;
}

// M[c] = sum_blk partial[blk][c] ; logits[k] = M . Wc[k] + bc[k]; one block of 256
__global__ void __launch_bounds__(256) pool_final_kernel(const float* __restrict__ partial, int nblk, int L,
                                                         const float* __restrict__ Wc, const float* __restrict__ bc,
                                                         int C, float* __restrict__ M, float* __restrict__ logits) {
  extern __shared__ float sm[];   // L floats of M + 4 reduction slots
  float* red = sm + L;
  for (int c = threadIdx.x; c < L; c += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += partial[(size_t)k * L + c];
    sm[c] = s;
    M[c] = s;
  }
  __syncthreads();
  for (int k = 0; k < C; ++k) {
    float s = 0.f;
    for (int c = threadIdx.x; c < L; c += blockDim.x) s += sm[c] * Wc[(size_t)k * L + c];
    s = block_reduce<false>(s, red);
    if (threadIdx.x == 0) logits[k] = s + bc[k];
  }
}

// dM = dl Wc, dWc = dl^T M, dbc = dl; one block of 256
__global__ void __launch_bounds__(256) bwd_head_kernel(const float* __restrict__ dl, const float* __restrict__ M,
                                                       const float* __restrict__ Wc, int C, int L,
                                                       float* __restrict__ dM, float* __restrict__ dWc,
                                                       float* __restrict__ dbc) {
  for (int c = threadIdx.x; c < L; c += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < C; ++k) {
      s += dl[k] * Wc[(size_t)k * L + c];
      dWc[(size_t)k * L + c] = dl[k] * M[c];
    }
    dM[c] = s;
  }
  if (threadIdx.x < C) dbc[threadIdx.x] = dl[threadIdx.x];
}

// one wave per row: dp_i = H_i . dM ; part[blk] = sum over the block's 4 rows of p_i dp_i
__global__ void __launch_bounds__(256) bwd_dp_kernel(const float* __restrict__ H, const float* __restrict__ dM,
                                                     const float* __restrict__ p, int N, int L,
                                                     float* __restrict__ dp, float* __restrict__ part) {
  __shared__ float red[4];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + wv;
  float v = 0.f;
  if (i < N) {
    const float* h = H + (size_t)i * L;
    float s = 0.f;
    for (int c = 4 * lane; c < L; c += 256) {
      const f32x4 x = *(const f32x4*)(h + c), g = *(const f32x4*)(dM + c);
      s += x[0] * g[0] + x[1] * g[1] + x[2] * g[2] + x[3] * g[3];
    }
    s = wave_sum(s);
    if (lane == 0) dp[i] = s;
    v = p[i] * s;
  }
  if (lane == 0) red[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// POOL_ROWS rows per block, one wave per row at a time: dZ, dH = p dM, and per-block dw / db partials
__global__ void __launch_bounds__(256) bwd_rows_kernel(const float* __restrict__ Z, const float* __restrict__ w,
                                                       const float* __restrict__ p, const float* __restrict__ dp,
                                                       const float* __restrict__ part, int npart,
                                                       const float* __restrict__ dM, int N, int D, int L,
                                                       float* __restrict__ dZ, float* __restrict__ dH,
                                                       float* __restrict__ dw_part, float* __restrict__ db_part) {
  extern __shared__ float sm[];   // 4 x D dw partials + 4 db + 4 reduction slots
  float* red = sm + 4 * D + 4;
  // S = sum_j p_j dp_j, summed in the same order by every block
  float s = 0.f;
  for (int k = threadIdx.x; k < npart; k += blockDim.x) s += part[k];
  const float S = block_reduce<false>(s, red);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * POOL_ROWS, r1 = min(N, r0 + POOL_ROWS);
  for (int d = lane; d < D; d += 64) sm[wv * D + d] = 0.f;
  float dbacc = 0.f;
  for (int i = r0 + wv; i < r1; i += 4) {
    const float pi = p[i], da = pi * (dp[i] - S);
    const float* z = Z + (size_t)i * 2 * D;
    float* gz = dZ + (size_t)i * 2 * D;
    for (int d = lane; d < D; d += 64) {
      const float t = tanhf(z[d]), sg = sigmoid_fast(z[D + d]), wd = w[d];
      gz[d] = da * wd * sg * (1.f - t * t);
      gz[D + d] = da * wd * t * sg * (1.f - sg);
      sm[wv * D + d] += da * t * sg;
    }
    dbacc += da;
    float* gh = dH + (size_t)i * L;
    for (int c = 4 * lane; c < L; c += 256) *(f32x4*)(gh + c) = pi * *(const f32x4*)(dM + c);
  }
  if (lane == 0) sm[4 * D + wv] = dbacc;
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    dw_part[(size_t)blockIdx.x * D + d] = sm[d] + sm[D + d] + sm[2 * D + d] + sm[3 * D + d];
  if (threadIdx.x == 0) db_part[blockIdx.x] = sm[4 * D] + sm[4 * D + 1] + sm[4 * D + 2] + sm[4 * D + 3];
}

// dw[d] = sum_blk dw_part[blk][d] ; db = sum_blk db_part[blk]; one block of 256
__global__ void __launch_bounds__(256) bwd_reduce_kernel(const float* __restrict__ dw_part,
                                                         const float* __restrict__ db_part, int nblk, int D,
                                                         float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[4];
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += dw_part[(size_t)k * D + d];
    dw[d] = s;
  }
  float s = 0.f;
  for (int k = threadIdx.x; k < nblk; k += blockDim.x) s += db_part[k];
  s = block_reduce<false>(s, red);
  if (threadIdx.x == 0) db[0] = s;
}

int nblk_rows(int N) { return (N + POOL_ROWS - 1) / POOL_ROWS; }

}  // namespace

extern "C" long long tm_attmil_fwd_workspace(int N, int L) {
  return (long long)(4 + (size_t)nblk_rows(N) * L) * sizeof(float);
}

extern "C" int tm_attmil_fwd(const float* Z, const float* H, const float* w, const float* b, const float* Wc,
                             const float* bc, int N, int L, int D, int C, float* work, float* a, float* p, float* M,
                             float* logits, void* stream) {
  TM_REQUIRE(N >= 1 && D >= 1 && C >= 1, "attmil_fwd: empty shape");
  TM_REQUIRE(L % 4 == 0 && L / 4 <= 1024, "attmil_fwd: L must be a multiple of 4, <= 4096");
  hipStream_t st = (hipStream_t)stream;
  float* stats = work;
  float* partial = work + 4;
  const int nblk = nblk_rows(N);
  score_kernel<<<(N + 3) / 4, 256, 0, st>>>(Z, N, D, w, b, a);
  stats_kernel<<<1, 1024, 0, st>>>(a, N, stats);
  pool_partial_kernel<<<nblk, L / 4, 0, st>>>(a, stats, H, N, L, p, partial);
  pool_final_kernel<<<1, 256, (L + 4) * sizeof(float), st>>>(partial, nblk, L, Wc, bc, C, M, logits);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_attmil_bwd_workspace(int N, int L, int D) {
  (void)L;
  return (long long)((size_t)(N + 3) / 4 + N + (size_t)nblk_rows(N) * (D + 1) + 4) * sizeof(float);
}

extern "C" int tm_attmil_bwd(const float* Z, const float* H, const float* w, const float* p, const float* M,
                             const float* Wc, const float* dlogits, int N, int L, int D, int C, float* work,
                             float* dZ, float* dH, float* dM, float* dw, float* db, float* dWc, float* dbc,
                             void* stream) {
  TM_REQUIRE(N >= 1 && D >= 1 && C >= 1 && C <= 256, "attmil_bwd: bad shape");
  TM_REQUIRE(L % 4 == 0, "attmil_bwd: L must be a multiple of 4");
  hipStream_t st = (hipStream_t)stream;
  const int npart = (N + 3) / 4, nblk = nblk_rows(N);
  float* part = work;                       // [npart] p_i dp_i partial sums
  float* dp = part + npart;                 // [N]
  float* dw_part = dp + N;                  // [nblk][D]
  float* db_part = dw_part + (size_t)nblk * D;   // [nblk]
  bwd_head_kernel<<<1, 256, 0, st>>>(dlogits, M, Wc, C, L, dM, dWc, dbc);
  bwd_dp_kernel<<<npart, 256, 0, st>>>(H, dM, p, N, L, dp, part);
  bwd_rows_kernel<<<nblk, 256, (4 * D + 8) * sizeof(float), st>>>(Z, w, p, dp, part, npart, dM, N, D, L, dZ, dH,
                                                                 dw_part, db_part);
  bwd_reduce_kernel<<<1, 256, 0, st>>>(dw_part, db_part, nblk, D, dw, db);
  TM_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The typed pooling (tm_attmil_pool_*): the same mathematics on Z / H / dZ rows stored as T = fp32
// or bf16 (the model's bf16 compute mode), fp32 arithmetic and fp32 everything else, in clam.hip's
// structure for its single-branch case.
// Forward, two stream-ordered launches:
//   pool_rows_fwd_kernel   PRB rows per workgroup.  A wave per row computes a_i from one read of the Z
//                          row (16-byte loads); the workgroup then takes its own maximum m_blk and
//                          s_blk = sum exp(a - m_blk) and adds exp(a - m_blk) H_i from one read of
//                          each H row.
//   pool_finalize_kernel   merges the block partials flash-style (m = max m_blk, each partial
//                          weighted by exp(m_blk - m)): stats = {m, s}, M, logits.
//   No exp of an unshifted score and no score-sized statistics pass.  a is saved; p is recomputed.
// Backward, three launches:
//   pool_bwd_head_kernel   dM = dl Wc, dWc = dl^T M, dbc = dl, r = M . dM (= sum_j p_j dp_j)
//   pool_rows_bwd_kernel   p_i = exp(a_i - m) / s, dp_i = H_i . dM, da_i = p_i (dp_i - r), dZ through
//                          tanh / sigmoid (stored as T), dH_i = p_i dM (fp32), block partials of dw / db
//   pool_bwd_reduce_kernel dw, db = the block partials added in block order
// No float atomics: every sum is a fixed tree or an index-ordered loop, so results repeat bitwise.
namespace {

constexpr int PRB = 64;           // rows per row-pass workgroup (tm_attmil_pool_rows_per_block)
constexpr int POOL_LMAX = 4096;   // L: width of H
constexpr int POOL_DMAX = 512;    // D: gate width (one 8-wide piece per lane of a wave)
constexpr int POOL_CMAX = 256;    // classes
constexpr int PFIN_THREADS = 1024;
static_assert(PRB == 64, "the block statistics take one score per lane of wave 0");

template <typename T>
__global__ void __launch_bounds__(256) pool_rows_fwd_kernel(const T* __restrict__ Z, const T* __restrict__ H,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            int N, int L, int D, float* __restrict__ a,
                                                            float* __restrict__ mb, float* __restrict__ sb,
                                                            float* __restrict__ part) {
  __shared__ float sc[PRB];                                        // scores, then exp(a - m_blk)
  __shared__ __attribute__((aligned(16))) float comb[256 * 8];     // the row groups' partial sums
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int r0 = blockIdx.x * PRB, nrows = min(N - r0, PRB);
  const float b0 = b[0];
  for (int j = wv; j < nrows; j += 4) {
    const T* z = Z + (size_t)(r0 + j) * 2 * D;
    float acc = 0.f;
    for (int d = 8 * lane; d < D; d += 512) {
      f32x8 th, sg;
      gate_parts8(load8f<T>(z + d), load8f<T>(z + D + d), th, sg);
      acc = dot8(th * sg, load8f<float>(w + d), acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      sc[j] = acc + b0;
      a[r0 + j] = acc + b0;
    }
  }
  __syncthreads();
  if (wv == 0) {
    const float v = lane < nrows ? sc[lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < nrows ? expf(v - m) : 0.f;
    const float s = wave_sum(e);
    if (lane < nrows) sc[lane] = e;
    if (lane == 0) {
      mb[blockIdx.x] = m;
      sb[blockIdx.x] = s;
    }
  }
  __syncthreads();
  // pooled partial: a thread owns one 8-column piece; with fewer than 256 pieces the rows are dealt
  // over G = 256 / pieces groups, whose sums are then added in group order
  const int nch = L / 8;
  const T* hb = H + (size_t)r0 * L;
  float* out = part + (size_t)blockIdx.x * L;
  if (nch >= 256) {
    for (int c = t; c < nch; c += 256) {
      f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int j = 0; j < nrows; ++j) acc += sc[j] * load8f<T>(hb + (size_t)j * L + 8 * c);
      store8<float>(out + 8 * c, acc);
    }
    return;
  }
  const int G = 256 / nch, g = t / nch, c = t - g * nch;
  f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (g < G) {
#pragma unroll 4
    for (int j = g; j < nrows; j += G) acc += sc[j] * load8f<T>(hb + (size_t)j * L + 8 * c);
    if (g > 0) store8<float>(comb + (size_t)(g * nch + c) * 8, acc);        // (g * nch + c) < 256
  }
  __syncthreads();
  if (g == 0) {
    for (int q = 1; q < G; ++q) acc += load8f<float>(comb + (size_t)(q * nch + c) * 8);
    store8<float>(out + 8 * c, acc);
  }
}

// One workgroup.  Slice q of the column groups adds the blocks q, q + S, ... in order; the S slices
// are then added in order.
__global__ void __launch_bounds__(PFIN_THREADS) pool_finalize_kernel(
    const float* __restrict__ mb, const float* __restrict__ sb, const float* __restrict__ part, int nblk, int L,
    const float* __restrict__ Wc, const float* __restrict__ bc, int C, float* __restrict__ stats,
    float* __restrict__ M, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float acc_s[POOL_LMAX];   // [S][L], S * L <= 4096
  __shared__ float Ms[POOL_LMAX];
  __shared__ float red[PFIN_THREADS / 64];
  const int t = threadIdx.x;
  float m = -INFINITY;
  for (int k = t; k < nblk; k += PFIN_THREADS) m = fmaxf(m, mb[k]);
  m = block_reduce<true, PFIN_THREADS / 64>(m, red);
  float s = 0.f;
  for (int k = t; k < nblk; k += PFIN_THREADS) s += sb[k] * expf(mb[k] - m);
  s = block_reduce<false, PFIN_THREADS / 64>(s, red);
  const int ncg = L / 4, S = PFIN_THREADS / ncg, slice = t / ncg, col = (t - slice * ncg) * 4;
  if (slice < S) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = slice; k < nblk; k += S) acc += expf(mb[k] - m) * *(const f32x4*)(part + (size_t)k * L + col);
    *(f32x4*)(acc_s + slice * L + col) = acc;
  }
  __syncthreads();
  for (int c = t; c < L; c += PFIN_THREADS) {
    float v = acc_s[c];
    for (int q = 1; q < S; ++q) v += acc_s[q * L + c];
    v /= s;
    M[c] = v;
    Ms[c] = v;
  }
  __syncthreads();
  const int wv = t >> 6, lane = t & 63;
  for (int k = wv; k < C; k += PFIN_THREADS / 64) {          // a wave per class
    float acc = 0.f;
    for (int c = lane; c < L; c += 64) acc = fmaf(Ms[c], Wc[(size_t)k * L + c], acc);
    acc = wave_sum(acc);
    if (lane == 0) logits[k] = acc + bc[k];
  }
  if (t == 0) {
    stats[0] = m;
    stats[1] = s;
  }
}

__global__ void __launch_bounds__(256) pool_bwd_head_kernel(const float* __restrict__ dl, const float* __restrict__ M,
                                                            const float* __restrict__ Wc, int C, int L,
                                                            float* __restrict__ dM, float* __restrict__ rv,
                                                            float* __restrict__ dWc, float* __restrict__ dbc) {
  __shared__ float red[4];
  float racc = 0.f;
  for (int c = threadIdx.x; c < L; c += 256) {
    const float mc = M[c];
    float s = 0.f;
    for (int k = 0; k < C; ++k) {
      s = fmaf(dl[k], Wc[(size_t)k * L + c], s);
      dWc[(size_t)k * L + c] = dl[k] * mc;
    }
    dM[c] = s;
    racc = fmaf(mc, s, racc);
  }
  const float r = block_reduce<false, 4>(racc, red);
  if (threadIdx.x == 0) rv[0] = r;
  for (int k = threadIdx.x; k < C; k += 256) dbc[k] = dl[k];
}

// PRB rows per workgroup, a wave per row.  LDS: dMs [L] | buf [4][D] | dbs [4]
template <typename T>
__global__ void __launch_bounds__(256) pool_rows_bwd_kernel(
    const T* __restrict__ Z, const T* __restrict__ H, const float* __restrict__ w, const float* __restrict__ a,
    const float* __restrict__ stats, const float* __restrict__ dM, const float* __restrict__ rv, int N, int L, int D,
    T* __restrict__ dZ, float* __restrict__ dH, float* __restrict__ dw_part, float* __restrict__ db_part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dMs = sm;
  float* buf = dMs + L;
  float* dbs = buf + 4 * D;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  for (int e = t; e < L; e += 256) dMs[e] = dM[e];
  __syncthreads();
  const float m = stats[0], inv = 1.f / stats[1], r = rv[0];
  const int r0 = blockIdx.x * PRB, r1 = min(N, r0 + PRB);
  const int d = 8 * lane;                                  // D <= 512: one 8-wide piece per lane
  f32x8 dwacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wd = dwacc;
  if (d < D) wd = load8f<float>(w + d);
  float dbacc = 0.f;
#pragma unroll 1
  for (int i = r0 + wv; i < r1; i += 4) {
    const T* h = H + (size_t)i * L;
    float dp = 0.f;
    for (int c = 8 * lane; c < L; c += 512) dp = dot8(load8f<T>(h + c), load8f<float>(dMs + c), dp);
    dp = wave_sum(dp);
    const float p = expf(a[i] - m) * inv, da = p * (dp - r);
    dbacc += da;
    float* gh = dH + (size_t)i * L;
    for (int c = 8 * lane; c < L; c += 512) store8<float>(gh + c, p * load8f<float>(dMs + c));
    if (d < D) {
      const T* z = Z + (size_t)i * 2 * D;
      T* gz = dZ + (size_t)i * 2 * D;
      f32x8 th, sg, ga, gb;
      gate_parts8(load8f<T>(z + d), load8f<T>(z + D + d), th, sg);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        dwacc[u] = fmaf(da, th[u] * sg[u], dwacc[u]);
        const GateGrad gg = gate_bwd(da * wd[u], th[u], sg[u]);
        ga[u] = gg.a;
        gb[u] = gg.b;
      }
      store8f<T>(gz + d, ga);
      store8f<T>(gz + D + d, gb);
    }
  }
  // the four waves' dw / db partials, added in wave order
  if (d < D) store8<float>(buf + wv * D + d, dwacc);
  if (lane == 0) dbs[wv] = dbacc;
  __syncthreads();
  for (int e = t; e < D; e += 256)
    dw_part[(size_t)blockIdx.x * D + e] = buf[e] + buf[D + e] + buf[2 * D + e] + buf[3 * D + e];
  if (t == 0) db_part[blockIdx.x] = dbs[0] + dbs[1] + dbs[2] + dbs[3];
}

// dw[e] / db = the block partials added in block order
__global__ void __launch_bounds__(256) pool_bwd_reduce_kernel(const float* __restrict__ dw_part,
                                                              const float* __restrict__ db_part, int nblk, int D,
                                                              float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < D) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += dw_part[(size_t)k * D + e];
    dw[e] = s;
  } else if (e == D) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += db_part[k];
    db[0] = s;
  }
}

int pool_nblk(int N) { return (N + PRB - 1) / PRB; }

const char* pool_check_shape(int dtype, int N, int L, int D, int C) {
  if (dtype != TM_F32 && dtype != TM_BF16) return "attmil_pool: dtype must be TM_F32 or TM_BF16";
  if (N < 1) return "attmil_pool: N must be >= 1";
  if (L < 8 || L % 8 != 0 || L > POOL_LMAX) return "attmil_pool: L must be a multiple of 8, <= 4096";
  if (D < 8 || D % 8 != 0 || D > POOL_DMAX) return "attmil_pool: D must be a multiple of 8, <= 512";
  if (C < 1 || C > POOL_CMAX) return "attmil_pool: C must be in [1, 256]";
  return nullptr;
}

bool pool_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int tm_attmil_pool_rows_per_block(void) { return PRB; }

extern "C" long long tm_attmil_pool_fwd_workspace(int N, int L) {
  if (N < 1 || L < 8 || L % 8 != 0 || L > POOL_LMAX) return 0;
  return (long long)pool_nblk(N) * (L + 2) * (long long)sizeof(float);
}

extern "C" int tm_attmil_pool_fwd(int dtype, const void* Z, const void* H, const float* w, const float* b,
                                  const float* Wc, const float* bc, int N, int L, int D, int C, float* work, float* a,
                                  float* stats, float* M, float* logits, void* stream) {
  const char* bad = pool_check_shape(dtype, N, L, D, C);
  TM_REQUIRE(bad == nullptr, bad);
  TM_REQUIRE(Z && H && w && b && Wc && bc && work && a && stats && M && logits, "attmil_pool_fwd: null pointer");
  TM_REQUIRE(pool_al16(Z) && pool_al16(H) && pool_al16(w) && pool_al16(Wc) && pool_al16(work) && pool_al16(a) &&
                 pool_al16(M),
             "attmil_pool_fwd: Z, H, w, Wc, work, a and M must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pool_nblk(N);
  float* part = work;                          // [nblk][L], 16-B aligned rows
  float* mb = part + (size_t)nblk * L;         // [nblk]
  float* sb = mb + nblk;                       // [nblk]
  if (dtype == TM_BF16)
    pool_rows_fwd_kernel<bf16><<<nblk, 256, 0, st>>>((const bf16*)Z, (const bf16*)H, w, b, N, L, D, a, mb, sb, part);
  else
    pool_rows_fwd_kernel<float><<<nblk, 256, 0, st>>>((const float*)Z, (const float*)H, w, b, N, L, D, a, mb, sb, part);
  pool_finalize_kernel<<<1, PFIN_THREADS, 0, st>>>(mb, sb, part, nblk, L, Wc, bc, C, stats, M, logits);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_attmil_pool_bwd_workspace(int N, int L, int D) {
  if (N < 1 || L < 8 || L % 8 != 0 || L > POOL_LMAX || D < 8 || D % 8 != 0 || D > POOL_DMAX) return 0;
  return ((long long)L + 4 + (long long)pool_nblk(N) * (D + 1)) * (long long)sizeof(float);
}

extern "C" int tm_attmil_pool_bwd(int dtype, const void* Z, const void* H, const float* w, const float* a,
                                  const float* stats, const float* M, const float* Wc, const float* dlogits, int N,
                                  int L, int D, int C, float* work, void* dZ, float* dH, float* dw, float* db,
                                  float* dWc, float* dbc, void* stream) {
  const char* bad = pool_check_shape(dtype, N, L, D, C);
  TM_REQUIRE(bad == nullptr, bad);
  TM_REQUIRE(Z && H && w && a && stats && M && Wc && dlogits && work && dZ && dH && dw && db && dWc && dbc,
             "attmil_pool_bwd: null pointer");
  TM_REQUIRE(pool_al16(Z) && pool_al16(H) && pool_al16(w) && pool_al16(a) && pool_al16(M) && pool_al16(Wc) &&
                 pool_al16(work) && pool_al16(dZ) && pool_al16(dH) && pool_al16(dw) && pool_al16(dWc),
             "attmil_pool_bwd: Z, H, w, a, M, Wc, work, dZ, dH, dw and dWc must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pool_nblk(N);
  float* dM = work;                            // [L]
  float* rv = dM + L;                          // [4]: r = M . dM
  float* dw_part = rv + 4;                     // [nblk][D]
  float* db_part = dw_part + (size_t)nblk * D; // [nblk]
  pool_bwd_head_kernel<<<1, 256, 0, st>>>(dlogits, M, Wc, C, L, dM, rv, dWc, dbc);
  const size_t lds = ((size_t)L + 4 * (size_t)D + 4) * sizeof(float);      // <= 24.1 KiB
  if (dtype == TM_BF16)
    pool_rows_bwd_kernel<bf16><<<nblk, 256, lds, st>>>((const bf16*)Z, (const bf16*)H, w, a, stats, dM, rv, N, L, D,
                                                       (bf16*)dZ, dH, dw_part, db_part);
  else
    pool_rows_bwd_kernel<float><<<nblk, 256, lds, st>>>((const float*)Z, (const float*)H, w, a, stats, dM, rv, N, L, D,
                                                        (float*)dZ, dH, dw_part, db_part);
  pool_bwd_reduce_kernel<<<(D + 1 + 255) / 256, 256, 0, st>>>(dw_part, db_part, nblk, D, dw, db);
  TM_CHECK_LAUNCH();
  return 0;
}
