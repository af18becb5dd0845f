// Moore-Penrose iterative pseudo-inverse (SURVEY.md App. A eq. 7) and the small
// batched fp32 products around it (Y = Z W and their backward).
//
// Replaces `moore_penrose_iter_pinv` of the third-party nystrom_attention
// package (called from NystromAttention.forward, code/models/TransMIL.py:47):
//   Z0 = X^T / (max_all rowsum|X| * max_all colsum|X|)      (maxima over ALL bags and heads)
//   6 x { P = X Z;  T3 = 15I - 7P + P P;  T5 = 13I - P T3;  Z = 0.25 Z T5 }
// (= 0.25 Z (13I - XZ(15I - XZ(7I - XZ))) with the inner product expanded).
// Forward schedule: P_{k+1} = X Z_{k+1} = 0.25 P_k T5_k = 3.25 P_k - 0.25 P_k^2 T3_k, so the
// P chain does not wait for Z: per iteration {R = P P with T3 = R - 7P + 15I as a second
// output of the same product, Z_k = 0.25 Z_{k-1} T5_{k-1}} then {T5 = 13I - P T3,
// P_{k+1} = 3.25 P - 0.25 R T3}: 2 dependent launches instead of 4 (14 in all instead of 24);
// the saved P / T3 / T5 / Z are the same tensors the backward uses.
//
// prec 0 (parity mode): exact fp32 on v_mfma_f32_32x32x2_f32 (fmaf chains); prec 1: the
// bf16x3 split of fp32 storage (the bench mode runs pinv_split.hip instead, which keeps
// the split planes in memory).  The attn2 entries sit in a ~5 % band around 1/256 and do
// not survive plain bf16.
// Every product is a 256x256(x64) fp32 batch over B*heads; one workgroup
// computes one 32x32 output tile with its 4 waves splitting K (reduced in LDS
// in a fixed order), batch index = blockIdx % nbatch so all tiles of one head
// land on one XCD (blocks b and b+8 share an XCD) and its 256 KB operands stay
// in that XCD's L2.
#include "common.h"
#include "../../include/transmil_hip.h"

#include <algorithm>

namespace {

constexpr int NL = 256;

struct JobPair { tm_bmm_job j[2]; int tiles0; };

// the bf16 form of an output element (tm_bmm_job.ct_mode): a copy, or split hi / lo planes
TM_DEV void store_ct(const tm_bmm_job& J, size_t off, float v) {
  if (J.ct_mode == 0) return;
  bf16* t = (bf16*)J.Ct;
  const bf16 hi = (bf16)v;
  t[off] = hi;
  if (J.ct_mode == 2) t[off + J.ct_plane] = (bf16)(v - (float)hi);
}



// the partial row dot of an output element's 32-column tile (tm_bmm_job.Rd): a row's 32 columns are
// the 32 lanes of one wave half (ln = lane, same register), summed by a fixed xor tree
TM_DEV void store_rowdot(const tm_bmm_job& J, int bh, int nbatch, int row, int col, float d, int ln) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if ((ln & 31) == 0) J.Rd[((size_t)(col / 32) * nbatch + bh) * J.M + row] = d;
}

TM_DEV f32x8 frag_a(const float* A, int ta, int lda, int m, int k) {
  if (ta == 0) return load8<float>(A + (size_t)m * lda + k);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = A[(size_t)(k + e) * lda + m];
  return r;
}
TM_DEV f32x8 frag_b(const float* B, int tb, int ldb, int k, int n) {
  if (tb == 1) return load8<float>(B + (size_t)n * ldb + k);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = B[(size_t)(k + e) * ldb + n];
  return r;
}

// One k-step (16 deep) of a 32x32 fp32 product.
//   PREC 0: exact fp32 (8 x v_mfma_f32_32x32x2_f32, an fmaf chain per element).
//   PREC 1: "bf16x3": x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (16 significant
//           bits); hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32
//           accumulation (dropped lo*lo ~ 2^-16 relative).  3 x 32 cycles instead of
//           8 x 64: used by the bf16 (bench) mode only.
template <int PREC>
TM_DEV void mma_f32_step(f32x16& acc, const f32x8& a, const f32x8& b) {
  if constexpr (PREC == 0) {
    mma16(acc, a, b);
  } else {
    bf16x8 ah, al, bh, bl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ah[e] = (bf16)a[e];
      al[e] = (bf16)(a[e] - (float)ah[e]);
      bh[e] = (bf16)b[e];
      bl[e] = (bf16)(b[e] - (float)bh[e]);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  }
}

// One workgroup = one 32x32 output tile of one batch entry; its 8 waves take the
// k-steps round-robin (s = wave, wave + 8, ...; every fragment requested before the
// first MFMA) and are summed in LDS in a fixed order.  4 waves per SIMD hide the L2
// latency of the operand loads behind each other's MFMAs.  (Generic layouts; the
// layout-specialised bmm_spec_kernel below serves every product the engine issues.)
constexpr int BMM_WAVES = 8;

template <int PREC>
__global__ __launch_bounds__(512) void bmm_kernel(JobPair jp, int nbatch) {
  __shared__ float red[BMM_WAVES][16][64];
  int b = blockIdx.x;
  const int which = b < jp.tiles0 * nbatch ? 0 : 1;
  if (which) b -= jp.tiles0 * nbatch;
  const tm_bmm_job& J = jp.j[which];
  const int bh = b % nbatch, tile = b / nbatch;
  const int ntn = J.N / 32;
  const int tm = tile / ntn, tn = tile % ntn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int nterms = J.A2 ? 2 : 1;
  const int nsteps = J.K * nterms / 16;
  f32x16 acc = (f32x16){};
  f32x8 af[4], bfr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int st = wave + BMM_WAVES * i;
    if (st < nsteps) {
      const int kk = st * 16;
      const int term = kk / J.K, kl = kk % J.K;
      const float* A = term ? J.A2 + bh * J.sa2 : J.A + bh * J.sa;
      const float* B = term ? J.B2 + bh * J.sb2 : J.B + bh * J.sb;
      const int ta = term ? J.ta2 : J.ta, tb = term ? J.tb2 : J.tb;
      const int lda = term ? J.lda2 : J.lda, ldb = term ? J.ldb2 : J.ldb;
      af[i] = frag_a(A, ta, lda, tm * 32 + r, kl + 8 * h);
      bfr[i] = frag_b(B, tb, ldb, kl + 8 * h, tn * 32 + r);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (wave + BMM_WAVES * i < nsteps) mma_f32_step<PREC>(acc, af[i], bfr[i]);
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 512 * q, reg = e >> 6, ln = e & 63;
    float s = red[0][reg][ln];
#pragma unroll
    for (int w = 1; w < BMM_WAVES; ++w) s += red[w][reg][ln];
    const int row = tm * 32 + acc_row(reg, ln >> 5), col = tn * 32 + (ln & 31);
    const size_t off = (size_t)bh * J.sc + (size_t)row * J.ldc + col;
    float v = J.alpha * s;
    if (row == col) v += J.diag;
    const float e1v = J.E1 ? J.E1[off] : 0.f;
    v += J.e1 * e1v;
    if (J.E2) v += J.e2 * J.E2[off];
    J.C[off] = v;
    if (J.C2) J.C2[off] = J.c2_alpha * s + (row == col ? J.c2_diag : 0.f) + J.c2_e1 * e1v;
    store_ct(J, off, v);
    if (J.Rd) store_rowdot(J, bh, nbatch, row, col, v * J.Rw[off], ln);
  }
}

// rowsum / colsum of |X|: grid (nbh, 2), block 256
__global__ void abs_sums_kernel(const float* __restrict__ X, float* __restrict__ sums, int nbh) {
  const int bh = blockIdx.x, t = threadIdx.x;
  const float* x = X + (size_t)bh * NL * NL;
  float s = 0.f;
  if (blockIdx.y == 0) {
    for (int j = 0; j < NL; ++j) s += fabsf(x[(size_t)t * NL + j]);
    sums[(size_t)bh * NL + t] = s;                       // rowsum ("col" in the package)
  } else {
    for (int i = 0; i < NL; ++i) s += fabsf(x[(size_t)i * NL + t]);
    sums[(size_t)(nbh + bh) * NL + t] = s;               // colsum ("row" in the package)
  }
}

struct MaxInfo { float maxc, maxr; float nc, nr; };

TM_DEV MaxInfo block_maxima(const float* sums, int nbh, float* red) {
  const int t = threadIdx.x, total = nbh * NL;
  float mc = -INFINITY, mr = -INFINITY;
  for (int i = t; i < total; i += 256) { mc = fmaxf(mc, sums[i]); mr = fmaxf(mr, sums[total + i]); }
  mc = wave_max(mc); mr = wave_max(mr);
  if ((t & 63) == 0) { red[t >> 6] = mc; red[4 + (t >> 6)] = mr; }
  __syncthreads();
  MaxInfo mi;
  mi.maxc = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  mi.maxr = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  __syncthreads();
  float nc = 0.f, nr = 0.f;
  for (int i = t; i < total; i += 256) { nc += sums[i] == mi.maxc; nr += sums[total + i] == mi.maxr; }
  nc = wave_sum(nc); nr = wave_sum(nr);
  if ((t & 63) == 0) { red[t >> 6] = nc; red[4 + (t >> 6)] = nr; }
  __syncthreads();
  mi.nc = red[0] + red[1] + red[2] + red[3];
  mi.nr = red[4] + red[5] + red[6] + red[7];
  __syncthreads();
  return mi;
}

// Z0[bh][i][j] = X[bh][j][i] / (maxc * maxr); grid (nbh, 16), block 256 (16 rows of Z0 each)
__global__ __launch_bounds__(256) void pinv_init_kernel(const float* __restrict__ X, const float* __restrict__ sums,
                                                        int nbh, float* __restrict__ Z0, float* __restrict__ stats) {
  __shared__ float red[8];
  __shared__ float tile[NL][17];
  const MaxInfo mi = block_maxima(sums, nbh, red);
  const float denom = mi.maxc * mi.maxr;
  const int bh = blockIdx.x, i0 = blockIdx.y * 16, t = threadIdx.x;
  const float* x = X + (size_t)bh * NL * NL;
  for (int e = t; e < NL * 16; e += 256) {
    const int j = e >> 4, ii = e & 15;
    tile[j][ii] = x[(size_t)j * NL + i0 + ii];          // X[j][i0+ii]
  }
  __syncthreads();
  for (int ii = 0; ii < 16; ++ii) Z0[((size_t)bh * NL + i0 + ii) * NL + t] = tile[t][ii] / denom;
  if (bh == 0 && blockIdx.y == 0 && t == 0) {
    stats[0] = mi.maxc; stats[1] = mi.maxr; stats[2] = denom; stats[3] = mi.nc; stats[4] = mi.nr;
  }
}

// partial sums of G0 * Z0 over 16-row slices: grid (nbh, 16)
__global__ void dot_partial_kernel(const float* __restrict__ G, const float* __restrict__ Z, float* __restrict__ part) {
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
// with dc = -sum(G0*Z0)/denom, dMc = dc*maxr, dMr = dc*maxc.  grid (nbh, 16)
__global__ __launch_bounds__(256) void pinv_init_bwd_kernel(const float* __restrict__ X, const float* __restrict__ sums,
                                                            const float* __restrict__ G0, const float* __restrict__ gz,
                                                            int nbh, float* __restrict__ dX) {
  __shared__ float red[8];
  __shared__ float tile[NL][17];
  const MaxInfo mi = block_maxima(sums, nbh, red);
  const float denom = mi.maxc * mi.maxr;
  const float dc = -gz[0] / denom;
  const float dMc = dc * mi.maxr / mi.nc, dMr = dc * mi.maxc / mi.nr;
  const int bh = blockIdx.x, i0 = blockIdx.y * 16, t = threadIdx.x;
  const float* g = G0 + (size_t)bh * NL * NL;
  for (int e = t; e < NL * 16; e += 256) {
    const int j = e >> 4, ii = e & 15;
    tile[j][ii] = g[(size_t)j * NL + i0 + ii];          // G0[j][i0+ii]
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

// ---------------------------------------------------------------------------
// Layout-specialised bmm.  The generic kernel above selects layouts and terms at run
// time; hipcc then branches around the fragment loads and waits for each group
// (s_waitcnt vmcnt between them) and reads the job fields with dependent loads from a
// dynamically indexed kernel argument: several serial memory round trips per launch.
// Here every job's layout, term count and k-slots are template constants, so each wave
// issues all of its fragment loads back to back and waits once.
// Layout code C: bit0 ta, bit1 tb, bit2 two terms (K = 256 each), bit3 ta2, bit4 tb2,
// bits5-6 slots per wave: 0 -> 2 (K = 256), 1 -> 1 (K <= 128), 2 -> 4 (two terms).
template <int TA>
TM_DEV f32x8 fa(const float* A, int lda, int m, int k) {
  if constexpr (TA == 0) return load8<float>(A + (size_t)m * lda + k);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = A[(size_t)(k + e) * lda + m];
  return r;
}
template <int TB>
TM_DEV f32x8 fb(const float* B, int ldb, int k, int n) {
  if constexpr (TB == 1) return load8<float>(B + (size_t)n * ldb + k);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = B[(size_t)(k + e) * ldb + n];
  return r;
}

template <int PREC, int C>
TM_DEV void bmm_tile(const tm_bmm_job& J, int bh, int tile, int nbatch, float (*red)[16][64]) {
  constexpr int TA = C & 1, TB = (C >> 1) & 1, TWO = (C >> 2) & 1, TA2 = (C >> 3) & 1, TB2 = (C >> 4) & 1;
  constexpr int SK = (C >> 5) & 3;
  constexpr int NSLOT = SK == 0 ? 2 : (SK == 1 ? 1 : 4);
  const int ntn = J.N / 32;
  const int m0 = (tile / ntn) * 32, n0 = (tile % ntn) * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  // epilogue operands first, so their latency overlaps the fragment loads
  float ev1[2] = {0.f, 0.f}, ev2[2] = {0.f, 0.f};
  size_t off[2];
  int row[2], col[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 512 * q, reg = e >> 6, ln = e & 63;
    row[q] = m0 + acc_row(reg, ln >> 5);
    col[q] = n0 + (ln & 31);
    off[q] = (size_t)bh * J.sc + (size_t)row[q] * J.ldc + col[q];
  }
  if (J.E1) { ev1[0] = J.E1[off[0]]; ev1[1] = J.E1[off[1]]; }
  if (J.E2) { ev2[0] = J.E2[off[0]]; ev2[1] = J.E2[off[1]]; }
  float rw[2] = {0.f, 0.f};
  if (J.Rd) { rw[0] = J.Rw[off[0]]; rw[1] = J.Rw[off[1]]; }
  f32x16 acc = (f32x16){};
  if (NSLOT > 1 || wave * 16 < J.K) {
    const float* A = J.A + bh * J.sa;
    const float* B = J.B + bh * J.sb;
    f32x8 af[NSLOT], bf[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int kk = (wave + 8 * i) * 16 + 8 * h;
      if constexpr (TWO) {
        if (i >= 2) {
          af[i] = fa<TA2>(J.A2 + bh * J.sa2, J.lda2, m0 + r, kk - 256);
          bf[i] = fb<TB2>(J.B2 + bh * J.sb2, J.ldb2, kk - 256, n0 + r);
          continue;
        }
      }
      af[i] = fa<TA>(A, J.lda, m0 + r, kk);
      bf[i] = fb<TB>(B, J.ldb, kk, n0 + r);
    }
    __builtin_amdgcn_sched_barrier(0);  // every fragment load is issued before the first MFMA waits
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) mma_f32_step<PREC>(acc, af[i], bf[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = tid + 512 * q, reg = e >> 6, ln = e & 63;
    float sum = red[0][reg][ln];
#pragma unroll
    for (int w = 1; w < BMM_WAVES; ++w) sum += red[w][reg][ln];
    float v = J.alpha * sum;
    if (row[q] == col[q]) v += J.diag;
    v += J.e1 * ev1[q] + J.e2 * ev2[q];
    J.C[off[q]] = v;
    if (J.C2) J.C2[off[q]] = J.c2_alpha * sum + (row[q] == col[q] ? J.c2_diag : 0.f) + J.c2_e1 * ev1[q];
    store_ct(J, off[q], v);
    if (J.Rd) store_rowdot(J, bh, nbatch, row[q], col[q], v * rw[q], ln);
  }
}

template <int PREC, int C0, int C1>
__global__ __launch_bounds__(512) void bmm_spec_kernel(JobPair jp, int nbatch) {
  __shared__ float red[BMM_WAVES][16][64];
  const int b = blockIdx.x;
  if (C1 < 0 || b < jp.tiles0 * nbatch) {
    bmm_tile<PREC, C0>(jp.j[0], b % nbatch, b / nbatch, nbatch, red);
  } else {
    const int b1 = b - jp.tiles0 * nbatch;
    bmm_tile<PREC, (C1 < 0 ? 0 : C1)>(jp.j[1], b1 % nbatch, b1 / nbatch, nbatch, red);
  }
}

int bmm_code(const tm_bmm_job& J) {
  if (J.A2) {
    if (J.K != 256) return -1;
    return (J.ta & 1) | (J.tb & 1) << 1 | 4 | (J.ta2 & 1) << 3 | (J.tb2 & 1) << 4 | 2 << 5;
  }
  if (J.K == 256) return (J.ta & 1) | (J.tb & 1) << 1;
  if (J.K <= 128 && J.K % 16 == 0) return (J.ta & 1) | (J.tb & 1) << 1 | 1 << 5;
  return -1;
}

template <int PREC>
bool launch_spec(const JobPair& jp, int c0, int c1, int total, int nbatch, hipStream_t st) {
#define TM_SPEC(A, B)                                                                  \
  if (c0 == A && c1 == B) {                                                            \
    bmm_spec_kernel<PREC, A, B><<<total, 512, 0, st>>>(jp, nbatch);                    \
    return true;                                                                       \
  }
  // single jobs: every layout at K = 256 and K <= 128, and the two-term dP update
  TM_SPEC(0, -1) TM_SPEC(1, -1) TM_SPEC(2, -1) TM_SPEC(3, -1)
  TM_SPEC(32, -1) TM_SPEC(33, -1) TM_SPEC(34, -1) TM_SPEC(35, -1) TM_SPEC(78, -1)
  // the job pairs of the pseudo-inverse backward and the landmark gradients
  TM_SPEC(1, 2) TM_SPEC(2, 1) TM_SPEC(34, 1) TM_SPEC(0, 1) TM_SPEC(0, 2) TM_SPEC(0, 0)
#undef TM_SPEC
  return false;
}

int launch_bmm(const tm_bmm_job* jobs, int njobs, int nbatch, int prec, hipStream_t st) {
  TM_REQUIRE(njobs == 1 || njobs == 2, "bmm: njobs must be 1 or 2");
  JobPair jp{};
  int total = 0;
  for (int i = 0; i < njobs; ++i) {
    const tm_bmm_job& J = jobs[i];
    TM_REQUIRE(J.A && J.B && J.C, "bmm: null operand");
    TM_REQUIRE(J.M % 32 == 0 && J.N % 32 == 0, "bmm: M, N must be multiples of 32");
    const int nterms = J.A2 ? 2 : 1;
    TM_REQUIRE(J.K % 16 == 0 && J.K * nterms <= 16 * BMM_WAVES * 4, "bmm: K must be a multiple of 16, K*terms <= 512");
    jp.j[i] = J;
    const int tiles = (J.M / 32) * (J.N / 32);
    if (i == 0) jp.tiles0 = tiles;
    total += tiles * nbatch;
  }
  const int c0 = bmm_code(jobs[0]), c1 = njobs > 1 ? bmm_code(jobs[1]) : -1;
  if (c0 >= 0 && (njobs == 1 || c1 >= 0)) {
    const bool ok = prec == 1 ? launch_spec<1>(jp, c0, c1, total, nbatch, st)
                              : launch_spec<0>(jp, c0, c1, total, nbatch, st);
    if (ok) {
      TM_CHECK_LAUNCH();
      return 0;
    }
  }
  if (prec == 1) bmm_kernel<1><<<total, 512, 0, st>>>(jp, nbatch);
  else bmm_kernel<0><<<total, 512, 0, st>>>(jp, nbatch);
  TM_CHECK_LAUNCH();
  return 0;
}

tm_bmm_job job(const float* A, int ta, const float* B, int tb, float* C, int M, int N, int K, float alpha,
               float diag = 0.f) {
  tm_bmm_job j{};
  j.A = A; j.ta = ta; j.B = B; j.tb = tb;
  j.lda = ta ? M : K;
  j.ldb = tb ? K : N;
  j.sa = (long long)M * K; j.sb = (long long)K * N;
  j.C = C; j.ldc = N; j.sc = (long long)M * N;
  j.M = M; j.N = N; j.K = K;
  j.alpha = alpha; j.diag = diag;
  return j;
}
void add_term(tm_bmm_job& j, const float* A, int ta, const float* B, int tb) {
  j.A2 = A; j.ta2 = ta; j.B2 = B; j.tb2 = tb;
  j.lda2 = ta ? j.M : j.K;
  j.ldb2 = tb ? j.K : j.N;
  j.sa2 = (long long)j.M * j.K; j.sb2 = (long long)j.K * j.N;
}

}  // namespace

#ifdef TM_DIAG
// Dispatch-placement probe for microbenchmarks only (not part of the supported ABI surface).
__global__ void xcc_map_kernel(int* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID[3:0]
}

// which XCD (0-7) each block of a `nblocks` x `threads` launch ran on (dispatch-placement probe)
extern "C" int tm_debug_xcc_map(int* out, int nblocks, int threads, void* stream) {
  TM_REQUIRE(out && nblocks > 0 && threads > 0 && threads <= 1024, "xcc_map: bad args");
  xcc_map_kernel<<<nblocks, threads, 0, (hipStream_t)stream>>>(out);
  TM_CHECK_LAUNCH();
  return 0;
}
#endif

extern "C" int tm_bmm(const tm_bmm_job* jobs, int njobs, int nbatch, int prec, void* stream) {
  TM_REQUIRE(prec == 0 || prec == 1, "bmm: prec must be 0 (fp32) or 1 (bf16x3)");
  return launch_bmm(jobs, njobs, nbatch, prec, (hipStream_t)stream);
}

// workspace: Zs[iters+1], Ps[iters], T3s[iters], T5s[iters] (each nbh*256*256 fp32) + sums[2][nbh][256] + stats[8]
extern "C" long long tm_pinv_saved_floats(int nbh, int iters) {
  return (4LL * iters + 1) * nbh * NL * NL + 2LL * nbh * NL + 8;
}

extern "C" int tm_pinv_fwd(const float* X, int nbh, int iters, int prec, float* saved, void* stream) {
  TM_REQUIRE(X && saved && iters >= 0, "pinv_fwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  const size_t mat = (size_t)nbh * NL * NL;
  float* Zs = saved;
  float* Ps = Zs + (iters + 1) * mat;
  float* T3s = Ps + iters * mat;
  float* T5s = T3s + iters * mat;
  float* sums = T5s + iters * mat;
  float* stats = sums + 2 * (size_t)nbh * NL;
  abs_sums_kernel<<<dim3(nbh, 2), 256, 0, st>>>(X, sums, nbh);
  TM_CHECK_LAUNCH();
  pinv_init_kernel<<<dim3(nbh, NL / 16), 256, 0, st>>>(X, sums, nbh, Zs, stats);
  TM_CHECK_LAUNCH();
  if (iters == 0) return 0;
  {
    tm_bmm_job j = job(X, 0, Zs, 0, Ps, NL, NL, NL, 1.f);              // P_0 = X Z_0
    if (int rc = launch_bmm(&j, 1, nbh, prec, st)) return rc;
  }
  for (int it = 0; it < iters; ++it) {
    float* P = Ps + it * mat;
    float* T3 = T3s + it * mat;
    float* T5 = T5s + it * mat;
    float* R = Zs + (it + 1) * mat;  // scratch: Z_{it+1} is written there after R's last read
    tm_bmm_job jb[2];
    jb[0] = job(P, 0, P, 0, R, NL, NL, NL, 1.f);                       // R = P P
    jb[0].E1 = P;
    jb[0].C2 = T3; jb[0].c2_alpha = 1.f; jb[0].c2_diag = 15.f; jb[0].c2_e1 = -7.f;  // T3 = R - 7P + 15I
    int nj = 1;
    if (it > 0)                                                        // Z_it = 0.25 Z_{it-1} T5_{it-1}
      jb[nj++] = job(Zs + (it - 1) * mat, 0, T5s + (it - 1) * mat, 0, Zs + it * mat, NL, NL, NL, 0.25f);
    if (int rc = launch_bmm(jb, nj, nbh, prec, st)) return rc;
    jb[0] = job(P, 0, T3, 0, T5, NL, NL, NL, -1.f, 13.f);              // T5 = 13I - P T3
    nj = 1;
    if (it + 1 < iters) {                                              // P_{it+1} = 3.25 P - 0.25 R T3
      jb[1] = job(R, 0, T3, 0, Ps + (it + 1) * mat, NL, NL, NL, -0.25f);
      jb[1].E1 = P; jb[1].e1 = 3.25f;
      nj = 2;
    }
    if (int rc = launch_bmm(jb, nj, nbh, prec, st)) return rc;
  }
  tm_bmm_job j = job(Zs + (iters - 1) * mat, 0, T5s + (iters - 1) * mat, 0, Zs + iters * mat, NL, NL, NL,
                     0.25f);                                           // Z_iters = 0.25 Z T5
  return launch_bmm(&j, 1, nbh, prec, st);
}

// workspace: 5 matrices + partial dots (nbh*16) + 1
extern "C" long long tm_pinv_bwd_workspace_floats(int nbh) {
  return 5LL * nbh * NL * NL + nbh * 16LL + 16;
}

// dZ (gradient w.r.t. the final Z) is consumed (overwritten).  dX is written (=).
extern "C" int tm_pinv_bwd(const float* X, int nbh, int iters, int prec, const float* saved, float* dZ, float* work,
                           float* dX, void* stream) {
  TM_REQUIRE(X && saved && dZ && work && dX, "pinv_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  const size_t mat = (size_t)nbh * NL * NL;
  const float* Zs = saved;
  const float* Ps = Zs + (iters + 1) * mat;
  const float* T3s = Ps + iters * mat;
  const float* T5s = T3s + iters * mat;
  const float* sums = T5s + iters * mat;
  float* dT5 = work;
  float* dZa = dT5 + mat;
  float* dP = dZa + mat;
  float* dT3 = dP + mat;
  float* part = dT3 + 2 * mat;  // (one spare matrix kept for alignment)
  float* gz = part + nbh * 16;
  float* G = dZ;
  bool first = true;
  for (int it = iters - 1; it >= 0; --it) {
    const float* Z = Zs + it * mat;
    const float* P = Ps + it * mat;
    const float* T3 = T3s + it * mat;
    const float* T5 = T5s + it * mat;
    tm_bmm_job jb[2];
    jb[0] = job(Z, 1, G, 0, dT5, NL, NL, NL, 0.25f);                    // dT5 = 0.25 Z^T G
    jb[1] = job(G, 0, T5, 1, dZa, NL, NL, NL, 0.25f);                   // dZa = 0.25 G T5^T
    if (int rc = launch_bmm(jb, 2, nbh, prec, st)) return rc;
    jb[0] = job(dT5, 0, T3, 1, dP, NL, NL, NL, -1.f);                   // dP  = -dT5 T3^T
    jb[1] = job(P, 1, dT5, 0, dT3, NL, NL, NL, -1.f);                   // dT3 = -P^T dT5
    if (int rc = launch_bmm(jb, 2, nbh, prec, st)) return rc;
    jb[0] = job(dT3, 0, P, 1, dP, NL, NL, NL, 1.f);                     // dP += dT3 P^T + P^T dT3 - 7 dT3
    add_term(jb[0], P, 1, dT3, 0);
    jb[0].E1 = dP; jb[0].e1 = 1.f; jb[0].E2 = dT3; jb[0].e2 = -7.f;
    if (int rc = launch_bmm(jb, 1, nbh, prec, st)) return rc;
    jb[0] = job(dP, 0, Z, 1, dX, NL, NL, NL, 1.f);                      // dX (+)= dP Z^T
    if (!first) { jb[0].E1 = dX; jb[0].e1 = 1.f; }
    jb[1] = job(X, 1, dP, 0, G, NL, NL, NL, 1.f);                       // G = dZa + X^T dP
    jb[1].E1 = dZa; jb[1].e1 = 1.f;
    if (int rc = launch_bmm(jb, 2, nbh, prec, st)) return rc;
    first = false;
  }
  if (first) {  // iters == 0: dX starts at zero
    if (hipMemsetAsync(dX, 0, mat * sizeof(float), st) != hipSuccess) { tm_set_error("pinv_bwd: memset"); return 2; }
  }
  // init: Z0 = X^T / (maxc * maxr)
  dot_partial_kernel<<<dim3(nbh, 16), 256, 0, st>>>(G, Zs, part);
  TM_CHECK_LAUNCH();
  if (int rc = tm_splitk_reduce(part, gz, nbh * 16, 1, 1.0f, 0, nullptr, stream)) return rc;   // read below
  pinv_init_bwd_kernel<<<dim3(nbh, 16), 256, 0, st>>>(X, sums, G, gz, nbh, dX);
  TM_CHECK_LAUNCH();
  return 0;
}
