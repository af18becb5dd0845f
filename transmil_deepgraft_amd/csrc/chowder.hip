// Chowder (code/models/Chowder.py:19-50): instance scores, two-sided top-R selection and the affine
// head, fp32 arithmetic on an fp32 or bf16 bag.
//   s[b,n]  = x[b,n,:] . w + bias                          (the 1x1 Conv1d(L, 1))
//   vals[b] = (R smallest of s[b,:] ascending, R largest descending), idx[b] the instance indices;
//             among equal scores the lower index is taken first, in both selections
//   h1 = W1 vals + b1 ; h2 = W2 h1 + b2 ; logits = W3 h2 + b3      (no non-linearity)
// Forward, two stream-ordered launches:
//   score_select_kernel  grid (chunks of CH rows, B): one wave per 4 rows, 16-byte loads, a wave sum;
//                        wave 0 then ranks the chunk's scores and writes its min(R, rows) smallest and
//                        largest (score, index) pairs, sorted, to the workspace
//   merge_head_kernel    grid B: R rounds of "the next pair after the last one taken" over the chunk
//                        candidates (in LDS when they fit, else read from the workspace), both
//                        selections per round; then the three affine layers in the same workgroup,
//                        8 lanes per output so that 128 weight rows are being read at once
// The launch boundary is the only hand-off between workgroups.
// Backward, two launches (plus a memset node for dx):
//   bwd_chain_kernel     one workgroup: dh2, dh1 (8 lanes per element), dvals (a wave per element)
//                        per bag, and the bias gradients
//   bwd_params_kernel    one thread per weight-gradient element / per column of dw, summing over the
//                        bags in order (b, then j); further workgroups write the selected rows of dx
// No float atomics anywhere: every sum has one fixed order, so results are bitwise repeatable.
#include "common.h"
#include "mil_common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int CH = 64;            // rows per chunk (= per score workgroup)
constexpr int ROWS_PER_WAVE = 4;  // rows a wave has in flight
constexpr int SCORE_THREADS = 64 * (CH / ROWS_PER_WAVE);   // 1024
constexpr int MERGE_THREADS = 1024;
constexpr int MERGE_WAVES = MERGE_THREADS / 64;
constexpr int STAGE_PAIRS = 6144;   // candidate pairs of one bag held in LDS (48 KiB); more are read in place
constexpr int MAX_R = 32;
constexpr int MAX_HID = 1024;       // H1, H2 (LDS copies of h1 / h2)

TM_DEV int chunks_of(int N) { return (N + CH - 1) / CH; }

// 8 consecutive features times 8 consecutive weights, added to acc one fmaf at a time
TM_DEV float dot8(const float* x, const float* w, float acc) {
  const f32x4 a = *(const f32x4*)x, b = *(const f32x4*)(x + 4);
  const f32x4 u = *(const f32x4*)w, v = *(const f32x4*)(w + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf(a[j], u[j], acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf(b[j], v[j], acc);
  return acc;
}
TM_DEV float dot8(const bf16* x, const float* w, float acc) {
  const bf16x8 a = *(const bf16x8*)x;
  const f32x4 u = *(const f32x4*)w, v = *(const f32x4*)(w + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf((float)a[j], u[j], acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf((float)a[4 + j], v[j], acc);
  return acc;
}

// Scores of one chunk and its candidates.  A row's sum: lane l adds the 8-feature groups l, l + 64,
// ... in order, then the wave's fixed butterfly; it depends on L alone.
template <typename T>
__global__ void __launch_bounds__(SCORE_THREADS) score_select_kernel(
    const T* __restrict__ x, int N, int L, const float* __restrict__ w, const float* __restrict__ bias, int R,
    float* __restrict__ scores, float* __restrict__ cand_v, int* __restrict__ cand_i) {
  __shared__ __attribute__((aligned(16))) float s[CH];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = chunk * CH + wave * ROWS_PER_WAVE;
  const T* xb = x + (size_t)b * N * L;
  const T* xr[ROWS_PER_WAVE];
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) xr[r] = xb + (size_t)min(row0 + r, N - 1) * L;   // clamped: read in bounds
  float acc[ROWS_PER_WAVE] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 8 * lane; c < L; c += 512) {
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) acc[r] = dot8(xr[r] + c, w + c, acc[r]);
  }
  const float bv = bias[0];
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const float v = wave_sum(acc[r]) + bv;
    if (lane == 0) {
      s[wave * ROWS_PER_WAVE + r] = v;      // rows past N: the clamped row's score, never counted below
      if (scores && row0 + r < N) scores[(size_t)b * N + row0 + r] = v;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const int nrow = min(CH, N - chunk * CH), cnt = min(R, nrow);
  if (lane >= nrow) return;
  const float si = s[lane];
  int below = 0, above = 0;     // rows that come before this one, ascending / descending, ties by index
#pragma unroll
  for (int j4 = 0; j4 < CH; j4 += 4) {      // 16 LDS broadcasts of four scores, all issued up front
    const f32x4 q = *(const f32x4*)(s + j4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j4 + u;
      const float sj = q[u];
      const bool in = j < nrow, first = sj == si && j < lane;
      below += (in && (sj < si || first)) ? 1 : 0;
      above += (in && (sj > si || first)) ? 1 : 0;
    }
  }
  const size_t base = ((size_t)b * nchunks + chunk) * 2 * R;
  if (below < cnt) {
    cand_v[base + below] = si;
    cand_i[base + below] = chunk * CH + lane;
  }
  if (above < cnt) {
    cand_v[base + R + above] = si;
    cand_i[base + R + above] = chunk * CH + lane;
  }
}

// sum_k A[k * sa] * v[k] over a group of GL neighbouring lanes: lane `sub` of the group adds k = sub,
// sub + GL, ... in order, then the group's xor butterfly (every lane of the group gets the sum).
// Every lane of the wave must call it (`on` false: contributes nothing); the loads of one lane are
// independent of each other, so many outputs are in flight at once instead of one per wave.
template <int GL>
TM_DEV float group_dot(const float* __restrict__ A, int sa, const float* v, int K, bool on) {
  const int sub = threadIdx.x & (GL - 1);
  float a = 0.f;
  if (on) {
#pragma unroll 8
    for (int k = sub; k < K; k += GL) a = fmaf(A[(size_t)k * sa], v[k], a);
  }
#pragma unroll
  for (int o = GL / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

constexpr int HEAD_GL = 8;    // lanes per output in the head

// out[j] = W[j,:] . in + bias[j] (in, out in LDS): 8 lanes per output, 128 outputs of the workgroup in
// flight.  Results stay in LDS; the kernel stores them to HBM once, at its end, so that no barrier
// on the way waits for a global store to be acknowledged.
TM_DEV void affine(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int K, int J,
                   float* out) {
  const int grp = threadIdx.x / HEAD_GL, sub = threadIdx.x & (HEAD_GL - 1);
  for (int j0 = 0; j0 < J; j0 += MERGE_THREADS / HEAD_GL) {
    const int j = j0 + grp;
    const bool on = j < J;
    const float a = group_dot<HEAD_GL>(W + (size_t)(on ? j : 0) * K, 1, in, K, on);
    if (on && sub == 0) out[j] = a + bias[j];
  }
  __syncthreads();
}

// R rounds over one bag's candidates: round k takes, on each side, the first pair in that side's order
// that comes after the pair taken in round k - 1.  cv / ci: [nchunks][2][R] (LDS or the workspace);
// sel / sel_i [2R] (LDS) receive the selected scores and indices.
TM_DEV void select_rounds(const float* cv, const int* ci, int nchunks, int N, int R, Pair (*red)[2][MERGE_WAVES],
                          float* sel, int* sel_i) {
  Pair last_lo = {-INFINITY, -1}, last_hi = {INFINITY, -1};
  for (int k = 0; k < R; ++k) {
    Pair lo = {INFINITY, INT_MAX}, hi = {-INFINITY, INT_MAX};
    for (int e = threadIdx.x; e < nchunks * R; e += MERGE_THREADS) {
      const int c = e / R, sl = e - c * R;
      if (sl >= min(R, N - c * CH)) continue;      // the last chunk may hold fewer than R rows
      const int at = c * 2 * R + sl;
      const float vl = cv[at], vh = cv[at + R];
      const int il = ci[at], ih = ci[at + R];
      if (before_min(last_lo.v, last_lo.i, Pair{vl, il}) && before_min(vl, il, lo)) lo = {vl, il};
      if (before_max(last_hi.v, last_hi.i, Pair{vh, ih}) && before_max(vh, ih, hi)) hi = {vh, ih};
    }
    const PairLoHi got = select_round_tail<MERGE_WAVES>(lo, hi, red[k & 1]);   // two buffers: one barrier per round
    last_lo = got.lo;
    last_hi = got.hi;
    if (threadIdx.x == 0) {
      sel[k] = got.lo.v;
      sel[R + k] = got.hi.v;
      sel_i[k] = select_clamp(got.lo.i, N);
      sel_i[R + k] = select_clamp(got.hi.i, N);
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(MERGE_THREADS) merge_head_kernel(
    const float* __restrict__ cand_v, const int* __restrict__ cand_i, int N, int R,
    const float* __restrict__ W1, const float* __restrict__ b1, int H1, const float* __restrict__ W2,
    const float* __restrict__ b2, int H2, const float* __restrict__ W3, const float* __restrict__ b3, int C,
    float* __restrict__ vals, int* __restrict__ idx, float* __restrict__ hid, float* __restrict__ logits) {
  __shared__ float cvs[STAGE_PAIRS];
  __shared__ int cis[STAGE_PAIRS];
  __shared__ Pair red[2][2][MERGE_WAVES];
  __shared__ float sel[2 * MAX_R];
  __shared__ int sel_i[2 * MAX_R];
  __shared__ float h1[MAX_HID];
  __shared__ float h2[MAX_HID];
  __shared__ float lg[MAX_HID];
  const int b = blockIdx.x, nchunks = chunks_of(N), npairs = nchunks * 2 * R;
  const float* cv = cand_v + (size_t)b * npairs;
  const int* ci = cand_i + (size_t)b * npairs;
  if (npairs <= STAGE_PAIRS) {
    // slots the score kernel did not write (a short last chunk) are copied as they are and never read
    for (int e = threadIdx.x; e < npairs; e += MERGE_THREADS) {
      cvs[e] = cv[e];
      cis[e] = ci[e];
    }
    __syncthreads();
    select_rounds(cvs, cis, nchunks, N, R, red, sel, sel_i);
  } else {
    select_rounds(cv, ci, nchunks, N, R, red, sel, sel_i);
  }
  affine(W1, b1, sel, 2 * R, H1, h1);
  affine(W2, b2, h1, H1, H2, h2);
  affine(W3, b3, h2, H2, C, lg);
  const int t = threadIdx.x;          // MERGE_THREADS >= 2 MAX_R and >= MAX_HID: one element per thread
  if (t < 2 * R) {
    vals[(size_t)b * 2 * R + t] = sel[t];
    idx[(size_t)b * 2 * R + t] = sel_i[t];
  }
  float* hb = hid + (size_t)b * (H1 + H2);
  if (t < H1) hb[t] = h1[t];
  if (t < H2) hb[H1 + t] = h2[t];
  if (t < C) logits[(size_t)b * C + t] = lg[t];
}

// dh2 = W3^T dl, dh1 = W2^T dh2, dvals = W1^T dh1 per bag, then the four bias gradients; one workgroup
__global__ void __launch_bounds__(1024) bwd_chain_kernel(
    const float* __restrict__ dl, int B, int R, const float* __restrict__ W1, int H1, const float* __restrict__ W2,
    int H2, const float* __restrict__ W3, int C, float* __restrict__ dh2, float* __restrict__ dh1,
    float* __restrict__ dvals, float* __restrict__ db, float* __restrict__ db1, float* __restrict__ db2,
    float* __restrict__ db3) {
  const int t = threadIdx.x, nt = blockDim.x, R2 = 2 * R;
  for (int e = t; e < B * H2; e += nt) {
    const int b = e / H2, j = e - b * H2;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(W3[(size_t)c * H2 + j], dl[(size_t)b * C + c], a);
    dh2[e] = a;
  }
  __syncthreads();
  for (int e0 = 0; e0 < B * H1; e0 += nt / 8) {        // 8 lanes per element of dh1
    const int e = e0 + t / 8;
    const bool on = e < B * H1;
    const int b = on ? e / H1 : 0, k = on ? e - b * H1 : 0;
    const float a = group_dot<8>(W2 + k, H1, dh2 + (size_t)b * H2, H2, on);
    if (on && (t & 7) == 0) dh1[e] = a;
  }
  __syncthreads();
  for (int e0 = 0; e0 < B * R2; e0 += nt / 64) {       // a wave per element of dvals
    const int e = e0 + t / 64;
    const bool on = e < B * R2;
    const int b = on ? e / R2 : 0, m = on ? e - b * R2 : 0;
    const float a = group_dot<64>(W1 + m, R2, dh1 + (size_t)b * H1, H1, on);
    if (on && (t & 63) == 0) dvals[e] = a;
  }
  __syncthreads();
  for (int e = t; e < C + H2 + H1 + 1; e += nt) {
    float a = 0.f;
    if (e < C) {
      for (int b = 0; b < B; ++b) a += dl[(size_t)b * C + e];
      db3[e] = a;
    } else if (e < C + H2) {
      const int j = e - C;
      for (int b = 0; b < B; ++b) a += dh2[(size_t)b * H2 + j];
      db2[j] = a;
    } else if (e < C + H2 + H1) {
      const int k = e - C - H2;
      for (int b = 0; b < B; ++b) a += dh1[(size_t)b * H1 + k];
      db1[k] = a;
    } else {
      for (int i = 0; i < B * R2; ++i) a += dvals[i];     // b, then j
      db[0] = a;
    }
  }
}

// Blocks [0, nparam): one thread per element of dW1 | dW2 | dW3 | dw, each a sum over the bags in order.
// Blocks [nparam, nparam + B * 2R) (only when dx): block (b, j) writes row idx[b,j] of dx, unless an
// earlier slot of the bag holds the same instance; the first slot writes the sum of both.
template <typename T>
__global__ void __launch_bounds__(256) bwd_params_kernel(
    const T* __restrict__ x, int B, int N, int L, const float* __restrict__ w, int R, int H1, int H2, int C,
    const float* __restrict__ vals, const int* __restrict__ idx, const float* __restrict__ hid,
    const float* __restrict__ dl, const float* __restrict__ dh2, const float* __restrict__ dh1,
    const float* __restrict__ dvals, int nparam, float* __restrict__ dw, float* __restrict__ dW1,
    float* __restrict__ dW2, float* __restrict__ dW3, float* __restrict__ dx) {
  const int R2 = 2 * R, HS = H1 + H2;
  if ((int)blockIdx.x >= nparam) {
    const int e = blockIdx.x - nparam, b = e / R2, j = e - b * R2;
    const int* ib = idx + (size_t)b * R2;
    const float* dv = dvals + (size_t)b * R2;
    const int row = ib[j];
    if (row < 0 || row >= N) return;
    float coef = 0.f;
    for (int q = 0; q < R2; ++q) {
      if (ib[q] != row) continue;
      if (q < j) return;
      coef += dv[q];
    }
    float* out = dx + ((size_t)b * N + row) * L;
    for (int c = 4 * threadIdx.x; c < L; c += 4 * blockDim.x) *(f32x4*)(out + c) = coef * *(const f32x4*)(w + c);
    return;
  }
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  float a = 0.f;
  if (e < H1 * R2) {
    const int k = e / R2, m = e - k * R2;
    for (int b = 0; b < B; ++b) a = fmaf(dh1[(size_t)b * H1 + k], vals[(size_t)b * R2 + m], a);
    dW1[e] = a;
    return;
  }
  e -= H1 * R2;
  if (e < H2 * H1) {
    const int j = e / H1, k = e - j * H1;
    for (int b = 0; b < B; ++b) a = fmaf(dh2[(size_t)b * H2 + j], hid[(size_t)b * HS + k], a);
    dW2[e] = a;
    return;
  }
  e -= H2 * H1;
  if (e < C * H2) {
    const int c = e / H2, j = e - c * H2;
    for (int b = 0; b < B; ++b) a = fmaf(dl[(size_t)b * C + c], hid[(size_t)b * HS + H1 + j], a);
    dW3[e] = a;
    return;
  }
  e -= C * H2;
  if (e < L) {
    for (int b = 0; b < B; ++b)
#pragma unroll 4
      for (int j = 0; j < R2; ++j) {
        const int row = idx[(size_t)b * R2 + j];
        if (row < 0 || row >= N) continue;
        a = fmaf(dvals[(size_t)b * R2 + j], to_f(x[((size_t)b * N + row) * L + e]), a);
      }
    dw[e] = a;
  }
}

const char* check_shape(int dtype, int B, int N, int L, int R, int H1, int H2, int C) {
  if (dtype != TM_F32 && dtype != TM_BF16) return "chowder: dtype must be TM_F32 or TM_BF16";
  if (B < 1 || B > 65535) return "chowder: B must be in [1, 65535]";
  if (L < 8 || L % 8 != 0 || L > 4096) return "chowder: L must be a multiple of 8, <= 4096";
  if (R < 1 || R > MAX_R) return "chowder: R must be in [1, 32]";
  if (N < R) return "chowder: N must be >= R (selected index out of range)";
  if (H1 < 1 || H2 < 1 || C < 1 || H1 > MAX_HID || H2 > MAX_HID || C > MAX_HID)
    return "chowder: H1, H2 and C must be in [1, 1024]";
  return nullptr;
}

}  // namespace

extern "C" long long tm_chowder_fwd_workspace(int B, int N, int L, int R) {
  (void)L;
  if (B < 1 || N < 1 || R < 1) return 0;
  return (long long)B * ((N + CH - 1) / CH) * 2 * R * (long long)(sizeof(float) + sizeof(int));
}

extern "C" int tm_chowder_fwd(int dtype, const void* x, int B, int N, int L, const float* w, const float* b, int R,
                              const float* W1, const float* b1, int H1, const float* W2, const float* b2, int H2,
                              const float* W3, const float* b3, int C, void* work, float* scores, float* vals,
                              int* idx, float* hid, float* logits, void* stream) {
  const char* bad = check_shape(dtype, B, N, L, R, H1, H2, C);
  TM_REQUIRE(bad == nullptr, bad);
  hipStream_t st = (hipStream_t)stream;
  const int nchunks = (N + CH - 1) / CH;
  const size_t npairs = (size_t)B * nchunks * 2 * R;
  float* cand_v = (float*)work;
  int* cand_i = (int*)(cand_v + npairs);
  const dim3 grid(nchunks, B);
  if (dtype == TM_BF16)
    score_select_kernel<bf16><<<grid, SCORE_THREADS, 0, st>>>((const bf16*)x, N, L, w, b, R, scores, cand_v, cand_i);
  else
    score_select_kernel<float><<<grid, SCORE_THREADS, 0, st>>>((const float*)x, N, L, w, b, R, scores, cand_v, cand_i);
  merge_head_kernel<<<B, MERGE_THREADS, 0, st>>>(cand_v, cand_i, N, R, W1, b1, H1, W2, b2, H2, W3, b3, C, vals, idx,
                                                 hid, logits);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_chowder_bwd_workspace(int B, int L, int R, int H1, int H2, int C) {
  (void)L;
  (void)C;
  if (B < 1 || R < 1 || H1 < 1 || H2 < 1) return 0;
  return (long long)B * (H2 + H1 + 2 * R) * (long long)sizeof(float);
}

extern "C" int tm_chowder_bwd(int dtype, const void* x, int B, int N, int L, const float* w, int R, const float* W1,
                              int H1, const float* W2, int H2, const float* W3, int C, const float* vals,
                              const int* idx, const float* hid, const float* dlogits, void* work, float* dw,
                              float* db, float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                              float* dx, void* stream) {
  const char* bad = check_shape(dtype, B, N, L, R, H1, H2, C);
  TM_REQUIRE(bad == nullptr, bad);
  hipStream_t st = (hipStream_t)stream;
  float* dh2 = (float*)work;
  float* dh1 = dh2 + (size_t)B * H2;
  float* dvals = dh1 + (size_t)B * H1;
  bwd_chain_kernel<<<1, 1024, 0, st>>>(dlogits, B, R, W1, H1, W2, H2, W3, C, dh2, dh1, dvals, db, db1, db2, db3);
  if (dx) {
    if (hipMemsetAsync(dx, 0, (size_t)B * N * L * sizeof(float), st) != hipSuccess) {
      tm_set_error("chowder_bwd: clearing dx failed");
      return 2;
    }
  }
  const int nelem = H1 * 2 * R + H2 * H1 + C * H2 + L;
  const int nparam = (nelem + 255) / 256;
  const int nblk = nparam + (dx ? B * 2 * R : 0);
  if (dtype == TM_BF16)
    bwd_params_kernel<bf16><<<nblk, 256, 0, st>>>((const bf16*)x, B, N, L, w, R, H1, H2, C, vals, idx, hid, dlogits,
                                                  dh2, dh1, dvals, nparam, dw, dW1, dW2, dW3, dx);
  else
    bwd_params_kernel<float><<<nblk, 256, 0, st>>>((const float*)x, B, N, L, w, R, H1, H2, C, vals, idx, hid, dlogits,
                                                   dh2, dh1, dvals, nparam, dw, dW1, dW2, dW3, dx);
  TM_CHECK_LAUNCH();
  return 0;
}
