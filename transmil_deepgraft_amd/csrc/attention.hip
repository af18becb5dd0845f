// Exact multi-head softmax attention, forward and backward, dim_head = 64, no mask
// (TransformerMIL's ViT blocks: code/models/_transformer.py:33-43, softmax(q k^T dh^-1/2) v).
//
// q / k / v are read in place from the packed to_qkv output ([B, n, 3*H*64] fp32, three base
// pointers and one row stride); the n x n scores are never written to memory.  Operands are
// rounded to T while they are staged (T = float: the fp32 MFMA, exact fmaf chains; T = bf16: the
// bf16 MFMA with fp32 accumulation); the softmax statistics are fp32 in both modes.
//
// One orientation serves all three kernels: the score tile is computed with the SUMMED-OVER index
// of the following product on the accumulator's rows (registers) and the owned index on the lane,
//   forward / dQ : S^T[key][query] = K Q^T      (wave owns 32 queries, sweeps the keys)
//   dK, dV       : S  [query][key] = Q K^T      (wave owns 32 keys, sweeps the queries)
// so P and dS feed the next MFMA as its B operand straight from the registers
// (acc_as_operand(), common.h) and the other operand is read column-wise from the row-major LDS
// image (frag_cols()).  The owned rows' statistics (running max / sum, lse, D) are per lane in
// the query-owning kernels: the online softmax is 32 fmax + one cross-half exchange per chunk.
//
// A workgroup is 4 waves x 32 owned rows; the swept side is staged 64 rows at a time (global ->
// registers one chunk ahead, registers -> LDS between two barriers).  Rows past n are staged as
// zeros; keys past n get probability 0.  No atomics: dQ comes from a pass that owns its query
// rows, dK / dV from a pass that owns its key rows (S and dP are recomputed in both), so every
// output element has one writer and a fixed summation order.
#include "common.h"
#include "../../include/transmil_hip.h"

namespace {

constexpr int ADH = 64;        // dim_head
constexpr int ACH = 64;        // rows of the swept side per staged chunk
constexpr int ALD = 72;        // LDS row stride in elements (16-B aligned rows; the +8 spreads banks)
constexpr int AWG_ROWS = 128;  // rows a workgroup owns (4 waves x 32)

template <typename T> TM_DEV float attn_exp(float x);
template <> TM_DEV float attn_exp<float>(float x) { return expf(x); }
template <> TM_DEV float attn_exp<bf16>(float x) { return __expf(x); }

// 64 x 64 fp32 tile (rows r0.. of a tensor with `stride` floats per row, already offset to the
// head's columns) in registers: thread t holds columns 4 (t & 15).. of rows (t >> 4) + 16 i.
struct AttnStage { f32x4 v[4]; };

TM_DEV void tile_load(AttnStage& s, const float* __restrict__ base, long long stride, int r0, int n, int tid) {
  const int c4 = (tid & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + (tid >> 4) + 16 * i;
    s.v[i] = row < n ? *(const f32x4*)(base + (size_t)row * stride + c4) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}
template <typename T> TM_DEV void tile_store(const AttnStage& s, T* img, int tid) {
  const int c4 = (tid & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    vec4<T> o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = from_f<T>(s.v[i][e]);
    store4<T>(img + ((tid >> 4) + 16 * i) * ALD + c4, o);
  }
}

// A fragment with the image's rows on the lanes: img[row0 + r][k0 + 8h + j]
template <typename T> TM_DEV vec8<T> frag_rows(const T* img, int row0, int k0, int r, int h) {
  return load8<T>(img + (row0 + r) * ALD + k0 + 8 * h);
}
// A fragment of the transposed image (column c0 + r on the lane) in the k order of an accumulator
// operand: element j of lane (r, h) = img[k0 + 8 (j >> 2) + 4 h + (j & 3)][c0 + r]  (acc_k_index)
template <typename T> TM_DEV vec8<T> frag_cols(const T* img, int k0, int c0, int lane);
template <> TM_DEV f32x8 frag_cols<float>(const float* img, int k0, int c0, int lane) {
  // eight 4-byte reads, a row of 32 columns per lane half: the halves sit 4 rows = 32 banks apart
  const float* p = img + (k0 + 4 * (lane >> 5)) * ALD + c0 + (lane & 31);
  f32x8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = p[((j & 3) + 8 * (j >> 2)) * ALD];
  return a;
}
template <> TM_DEV bf16x8 frag_cols<bf16>(const bf16* img, int k0, int c0, int lane) {
  // two transposing reads of 4 rows x 16 columns per 16 lanes (as nystrom.hip's frag_tr_rows)
  const int g = lane >> 4, qd = (lane & 15) >> 2, p = lane & 3;
  const int c = c0 + (g & 1) * 16 + 4 * p;
  const int kk = k0 + 4 * (g >> 1) + qd;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(img + kk * ALD + c));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(img + (kk + 8) * ALD + c));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// B fragments of one fp32 row of global memory (the owned row of this lane): f[ks][j] = row[16 ks + 8h + j]
template <typename T> TM_DEV void frag_global(vec8<T> (&f)[4], const float* __restrict__ row, bool valid, int h) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (valid) {
      f[ks] = cvt8<T>(row + 16 * ks + 8 * h);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[ks][j] = from_f<T>(0.f);
    }
  }
}
// one owned row's 64 outputs: registers 4g..4g+3 of tile dt are columns 32 dt + 8g + 4h + 0..3
TM_DEV void store_row(float* __restrict__ row, const f32x16& t0, const f32x16& t1, float mul, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(f32x4*)(row + 8 * g + 4 * h) = (f32x4){t0[4 * g] * mul, t0[4 * g + 1] * mul, t0[4 * g + 2] * mul, t0[4 * g + 3] * mul};
    *(f32x4*)(row + 32 + 8 * g + 4 * h) =
        (f32x4){t1[4 * g] * mul, t1[4 * g + 1] * mul, t1[4 * g + 2] * mul, t1[4 * g + 3] * mul};
  }
}
TM_DEV f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// grid (ceil(n / 128), B*H), block 256
template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, int H, int n, long long rs,
                                                       float scale, float* __restrict__ out,
                                                       float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) T Ks[ACH * ALD];
  __shared__ __attribute__((aligned(16))) T Vs[ACH * ALD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const size_t boff = (size_t)b * n * rs + (size_t)hd * ADH;
  const float* kb = k + boff;
  const float* vb = v + boff;
  const int q0 = blockIdx.x * AWG_ROWS + wave * 32;
  const bool active = q0 < n;             // wave-uniform: a wave without rows only stages
  const int qrow = q0 + r;
  const bool qvalid = qrow < n;
  vec8<T> Qf[4];
  frag_global<T>(Qf, q + boff + (size_t)(qvalid ? qrow : 0) * rs, qvalid, h);
  f32x16 O0 = zero16(), O1 = zero16();
  float m = -INFINITY, l = 0.f;           // running max (whole row) and this lane half's part of the sum
  const int nchunks = (n + ACH - 1) / ACH;
  AttnStage sk, sv;
  tile_load(sk, kb, rs, 0, n, tid);
  tile_load(sv, vb, rs, 0, n, tid);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
    tile_store<T>(sk, Ks, tid);
    tile_store<T>(sv, Vs, tid);
    __syncthreads();
    if (c + 1 < nchunks) {
      tile_load(sk, kb, rs, (c + 1) * ACH, n, tid);
      tile_load(sv, vb, rs, (c + 1) * ACH, n, tid);
    }
    if (!active) continue;
    f32x16 S0 = zero16(), S1 = zero16();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      mma16(S0, frag_rows<T>(Ks, 0, 16 * ks, r, h), Qf[ks]);
      mma16(S1, frag_rows<T>(Ks, 32, 16 * ks, r, h), Qf[ks]);
    }
    const int kbase = c * ACH;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S0[i] *= scale; S1[i] *= scale; }
    if (kbase + ACH > n) {                 // the last chunk's tail keys
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (kbase + acc_row(i, h) >= n) S0[i] = -INFINITY;
        if (kbase + 32 + acc_row(i, h) >= n) S1[i] = -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, fmaxf(S0[i], S1[i]));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);         // finite: every chunk holds at least one key < n
    const float alpha = attn_exp<T>(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      S0[i] = attn_exp<T>(S0[i] - mn);
      S1[i] = attn_exp<T>(S1[i] - mn);
      ps += S0[i] + S1[i];
    }
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int i = 0; i < 16; ++i) { O0[i] *= alpha; O1[i] *= alpha; }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const vec8<T> p0 = acc_as_operand<T>(S0, s), p1 = acc_as_operand<T>(S1, s);
      mma16(O0, frag_cols<T>(Vs, 16 * s, 0, lane), p0);
      mma16(O1, frag_cols<T>(Vs, 16 * s, 32, lane), p0);
      mma16(O0, frag_cols<T>(Vs, 32 + 16 * s, 0, lane), p1);
      mma16(O1, frag_cols<T>(Vs, 32 + 16 * s, 32, lane), p1);
    }
  }
  if (!active) return;
  l += __shfl_xor(l, 32, 64);
  if (qvalid) {
    store_row(out + ((size_t)b * n + qrow) * ((size_t)H * ADH) + (size_t)hd * ADH, O0, O1, 1.f / l, h);
    if (h == 0) lse[(size_t)bh * n + qrow] = m + logf(l);
  }
}

// D[bh][t] = sum_d dout[b][t][h][d] * out[b][t][h][d]: 16 lanes per row, fixed butterfly order.
// grid ceil(B*n*H / 16), block 256
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                         int H, int n, long long rows, float* __restrict__ dvec) {
  const long long idx = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);   // (b*n + t)*H + h
  const int sub = threadIdx.x & 15;
  float s = 0.f;
  if (idx < rows) {
    const f32x4 a = *(const f32x4*)(out + (size_t)idx * ADH + sub * 4);
    const f32x4 d = *(const f32x4*)(dout + (size_t)idx * ADH + sub * 4);
    s = (a[0] * d[0] + a[1] * d[1]) + (a[2] * d[2] + a[3] * d[3]);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (sub == 0 && idx < rows) {
    const long long bt = idx / H;
    const int hd = (int)(idx % H);
    const long long b = bt / n, t = bt % n;
    dvec[((size_t)b * H + hd) * n + t] = s;
  }
}

// dQ = scale * dS K over the wave's 32 query rows.  grid (ceil(n / 128), B*H), block 256
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ dvec,
                                                          int H, int n, long long rs, float scale,
                                                          float* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) T Ks[ACH * ALD];
  __shared__ __attribute__((aligned(16))) T Vs[ACH * ALD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const size_t boff = (size_t)b * n * rs + (size_t)hd * ADH;
  const size_t hdim = (size_t)H * ADH;
  const float* kb = k + boff;
  const float* vb = v + boff;
  const int q0 = blockIdx.x * AWG_ROWS + wave * 32;
  const bool active = q0 < n;
  const int qrow = q0 + r;
  const bool qvalid = qrow < n;
  const size_t qr = qvalid ? qrow : 0;
  vec8<T> Qf[4], dOf[4];
  frag_global<T>(Qf, q + boff + qr * rs, qvalid, h);
  frag_global<T>(dOf, dout + ((size_t)b * n + qr) * hdim + (size_t)hd * ADH, qvalid, h);
  const float lse_q = qvalid ? lse[(size_t)bh * n + qrow] : 0.f;
  const float d_q = qvalid ? dvec[(size_t)bh * n + qrow] : 0.f;
  f32x16 G0 = zero16(), G1 = zero16();
  const int nchunks = (n + ACH - 1) / ACH;
  AttnStage sk, sv;
  tile_load(sk, kb, rs, 0, n, tid);
  tile_load(sv, vb, rs, 0, n, tid);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
    tile_store<T>(sk, Ks, tid);
    tile_store<T>(sv, Vs, tid);
    __syncthreads();
    if (c + 1 < nchunks) {
      tile_load(sk, kb, rs, (c + 1) * ACH, n, tid);
      tile_load(sv, vb, rs, (c + 1) * ACH, n, tid);
    }
    if (!active) continue;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        mma16(S, frag_rows<T>(Ks, 32 * kt, 16 * ks, r, h), Qf[ks]);
        mma16(dP, frag_rows<T>(Vs, 32 * kt, 16 * ks, r, h), dOf[ks]);
      }
      const int kbase = c * ACH + 32 * kt;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = kbase + acc_row(i, h) < n ? attn_exp<T>(S[i] * scale - lse_q) : 0.f;
        S[i] = p * (dP[i] - d_q);            // dS^T[key][query]
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const vec8<T> ds = acc_as_operand<T>(S, s);
        mma16(G0, frag_cols<T>(Ks, 32 * kt + 16 * s, 0, lane), ds);
        mma16(G1, frag_cols<T>(Ks, 32 * kt + 16 * s, 32, lane), ds);
      }
    }
  }
  if (active && qvalid)
    store_row(dqkv + ((size_t)b * n + qrow) * (3 * hdim) + (size_t)hd * ADH, G0, G1, scale, h);
}

// dV = P^T dO and dK = scale * dS^T Q over the wave's 32 key rows.  grid (ceil(n / 128), B*H), block 256
// (two waves per SIMD asked for: the fp32 form otherwise takes 259 registers, three over the limit
// for a second workgroup per CU, and one wave per SIMD leaves the MFMA idle during its softmax)
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ dvec,
                                                           int H, int n, long long rs, float scale,
                                                           float* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) T Qs[ACH * ALD];
  __shared__ __attribute__((aligned(16))) T dOs[ACH * ALD];
  __shared__ __attribute__((aligned(16))) float lse_s[ACH];
  __shared__ __attribute__((aligned(16))) float d_s[ACH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, hd = bh % H;
  const size_t boff = (size_t)b * n * rs + (size_t)hd * ADH;
  const size_t hdim = (size_t)H * ADH;
  const float* qb = q + boff;
  const float* dob = dout + (size_t)b * n * hdim + (size_t)hd * ADH;
  const float* lseb = lse + (size_t)bh * n;
  const float* dvb = dvec + (size_t)bh * n;
  const int k0 = blockIdx.x * AWG_ROWS + wave * 32;
  const bool active = k0 < n;
  const int krow = k0 + r;
  const bool kvalid = krow < n;
  const size_t kr = kvalid ? krow : 0;
  vec8<T> Kf[4], Vf[4];
  frag_global<T>(Kf, k + boff + kr * rs, kvalid, h);
  frag_global<T>(Vf, v + boff + kr * rs, kvalid, h);
  f32x16 dV0 = zero16(), dV1 = zero16(), dK0 = zero16(), dK1 = zero16();
  const int nchunks = (n + ACH - 1) / ACH;
  AttnStage sq, sd;
  float sl = INFINITY, sdv = 0.f;          // a padded query row: lse = +inf makes its P exactly 0
  tile_load(sq, qb, rs, 0, n, tid);
  tile_load(sd, dob, (long long)hdim, 0, n, tid);
  if (tid < ACH && tid < n) { sl = lseb[tid]; sdv = dvb[tid]; }
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
    tile_store<T>(sq, Qs, tid);
    tile_store<T>(sd, dOs, tid);
    if (tid < ACH) { lse_s[tid] = sl; d_s[tid] = sdv; }
    __syncthreads();
    if (c + 1 < nchunks) {
      const int r0 = (c + 1) * ACH;
      tile_load(sq, qb, rs, r0, n, tid);
      tile_load(sd, dob, (long long)hdim, r0, n, tid);
      if (tid < ACH) {
        const bool ok = r0 + tid < n;
        sl = ok ? lseb[r0 + tid] : INFINITY;
        sdv = ok ? dvb[r0 + tid] : 0.f;
      }
    }
    if (!active) continue;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x16 S = zero16(), dP = zero16();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        mma16(S, frag_rows<T>(Qs, 32 * qt, 16 * ks, r, h), Kf[ks]);
        mma16(dP, frag_rows<T>(dOs, 32 * qt, 16 * ks, r, h), Vf[ks]);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 L = *(const f32x4*)(lse_s + 32 * qt + 8 * g + 4 * h);
        const f32x4 Dd = *(const f32x4*)(d_s + 32 * qt + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = attn_exp<T>(S[4 * g + e] * scale - L[e]);
          dP[4 * g + e] = p * (dP[4 * g + e] - Dd[e]);   // dS[query][key]
          S[4 * g + e] = p;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const vec8<T> pp = acc_as_operand<T>(S, s), ds = acc_as_operand<T>(dP, s);
        mma16(dV0, frag_cols<T>(dOs, 32 * qt + 16 * s, 0, lane), pp);
        mma16(dV1, frag_cols<T>(dOs, 32 * qt + 16 * s, 32, lane), pp);
        mma16(dK0, frag_cols<T>(Qs, 32 * qt + 16 * s, 0, lane), ds);
        mma16(dK1, frag_cols<T>(Qs, 32 * qt + 16 * s, 32, lane), ds);
      }
    }
  }
  if (active && kvalid) {
    float* row = dqkv + ((size_t)b * n + krow) * (3 * hdim) + (size_t)hd * ADH;
    store_row(row + hdim, dK0, dK1, scale, h);
    store_row(row + 2 * hdim, dV0, dV1, 1.f, h);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the argument checks shared by the two entry points; 0 = fine (message set otherwise)
int attn_check_dims(int compute, int B, int H, int n, long long row_stride) {
  TM_REQUIRE(compute == TM_F32 || compute == TM_BF16, "attn: compute must be TM_F32 or TM_BF16");
  TM_REQUIRE(n > 0, "attn: n must be positive");
  TM_REQUIRE(B > 0, "attn: B must be positive");
  TM_REQUIRE(H > 0, "attn: H must be positive");
  TM_REQUIRE((long long)B * H <= 65535, "attn: B*H must be at most 65535");
  TM_REQUIRE(row_stride >= (long long)H * ADH, "attn: row_stride must be at least H*64");
  TM_REQUIRE(row_stride % 4 == 0, "attn: row_stride must be a multiple of 4");
  return 0;
}

long long attn_delta_bytes(int B, int H, int n) { return ((long long)B * H * n * 4 + 255) / 256 * 256; }

}  // namespace

extern "C" int tm_attn_fwd(int compute, const float* q, const float* k, const float* v, int B, int H, int n,
                           long long row_stride, float scale, float* out, float* lse, void* stream) {
  if (int rc = attn_check_dims(compute, B, H, n, row_stride)) return rc;
  TM_REQUIRE(q && k && v && out && lse, "attn_fwd: null pointer");
  TM_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(lse),
             "attn_fwd: pointers must be 16-byte aligned");
  const dim3 grid((n + AWG_ROWS - 1) / AWG_ROWS, B * H);
  hipStream_t st = (hipStream_t)stream;
  if (compute == TM_BF16)
    attn_fwd_kernel<bf16><<<grid, 256, 0, st>>>(q, k, v, H, n, row_stride, scale, out, lse);
  else
    attn_fwd_kernel<float><<<grid, 256, 0, st>>>(q, k, v, H, n, row_stride, scale, out, lse);
  TM_CHECK_LAUNCH();
  return 0;
}

extern "C" long long tm_attn_bwd_workspace(int B, int H, int n) {
  if (B <= 0 || H <= 0 || n <= 0) return 0;
  return attn_delta_bytes(B, H, n);
}

extern "C" int tm_attn_bwd(int compute, const float* q, const float* k, const float* v, const float* out,
                           const float* lse, const float* dout, int B, int H, int n, long long row_stride,
                           float scale, void* work, float* dqkv, void* stream) {
  if (int rc = attn_check_dims(compute, B, H, n, row_stride)) return rc;
  TM_REQUIRE(q && k && v && out && lse && dout && work && dqkv, "attn_bwd: null pointer");
  TM_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(lse) && aligned16(dout) &&
                 aligned16(work) && aligned16(dqkv),
             "attn_bwd: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* dvec = (float*)work;
  const long long rows = (long long)B * n * H;
  TM_REQUIRE((rows + 15) / 16 <= 0x7fffffffLL, "attn_bwd: B*n*H too large");
  attn_delta_kernel<<<dim3((unsigned)((rows + 15) / 16)), 256, 0, st>>>(out, dout, H, n, rows, dvec);
  TM_CHECK_LAUNCH();
  const dim3 grid((n + AWG_ROWS - 1) / AWG_ROWS, B * H);
  if (compute == TM_BF16) {
    attn_bwd_dkv_kernel<bf16><<<grid, 256, 0, st>>>(q, k, v, dout, lse, dvec, H, n, row_stride, scale, dqkv);
    attn_bwd_dq_kernel<bf16><<<grid, 256, 0, st>>>(q, k, v, dout, lse, dvec, H, n, row_stride, scale, dqkv);
  } else {
    attn_bwd_dkv_kernel<float><<<grid, 256, 0, st>>>(q, k, v, dout, lse, dvec, H, n, row_stride, scale, dqkv);
    attn_bwd_dq_kernel<float><<<grid, 256, 0, st>>>(q, k, v, dout, lse, dvec, H, n, row_stride, scale, dqkv);
  }
  TM_CHECK_LAUNCH();
  return 0;
}
