// NystromAttention core, bench mode (bf16 operands on the bf16 MFMA, fp32 accumulation and
// softmax): the kernels the training step runs.  Included by nystrom.hip (the one translation
// unit) after nystrom_common.h and the kernels both modes share; the fp32 parity pipeline for
// the same maths is nystrom_f32.h.
//
// Kernels
//   a1_fwd_bf16_kernel       softmax(q kl^T) Y + conv33(v) -> merged rows: one workgroup per CU walks
//                            32-query chunks, the conv on the MFMA over an LDS-DMA v window
//   a3_fwd_v2_kernel         W partials = softmax(ql k^T) v over an even key split, online softmax;
//                            <ST, S2R>: S2R > 0 also writes the head's A2 rows (sim2_wave_rows)
//   a3_combine_v2_kernel     merge of those partials (a3_combine.h; the step runs the same routine
//                            inside the pseudo-inverse chain's last launch)
//   conv_bwd_mfma_kernel     conv33 backward + D1 on the MFMA, dv written bf16
//   attn_bwd_bf16_kernel     <MODE, NW, ST>: flash-style backward of the A1 / A3 products with every
//                            operand staged once (BwdLayT<NW, MQ>: BwdLay16, BwdLay9) and the fused
//                            epilogues (dq / k / v straight into dqkv, bf16 partial slabs)
// Diagnostic build only (TM_DIAG): the stamped instantiations of these kernels (s_memtime into
// g_a1_stamps), picked by NysSel.
#pragma once
#include <algorithm>
#include <type_traits>
#include "nystrom_common.h"
#include "a3_combine.h"

namespace {

// ---------------------------------------------------------------------------
// A1 path forward, bf16 (bench mode): one workgroup of 8 waves per CU; the landmark keys
// and Y are staged ONCE per workgroup and each wave walks 32-query chunks of its head.
// grid = (W, nbh) with W = min(256 / nbh, n / 32) workgroups per head and the head's n / 32
// chunks split evenly over them, so at N = 8192 every CU holds one workgroup (the
// 128-query-per-workgroup form launched 528 blocks on 512 slots: a second round for 16).
// The 33-tap residual conv runs on the MFMA: per chunk (queries t0..t0+31)
//   O^T[d][q] += sum_j V[t0 - 16 + j][d] * band[j][q],  band[j][q] = w[j - q] (0 <= j - q < 33)
// over the workgroup's v window: rows [32 c_begin - 16, 32 c_end + 16) copied HBM -> LDS by
// LDS-DMA (global_load_lds, no VGPRs) in the prologue and left in flight through the first
// attention phase (v is read 1.1-1.2x, not the 2x of per-chunk windows).  Rows outside
// [0, n) are fetched clamped and masked in the band instead.  The band fragments of
// interior chunks are one shared LDS table; the first / last chunk of a head build theirs.
// LDS: keys [256][72] + Y [256][80] + window [<=320][64] + 4 output stages [32][72] + band
// table + taps = 140 KB.  One wave per SIMD (512 registers): the wave overlaps its own MFMA
// and VALU work instead of two waves running the same phases in lockstep.
constexpr int A1P_WAVES = 4;                                            // one wave per SIMD: 512 registers
constexpr int A1P_MAXCH = 9;                                            // chunks per workgroup (host-checked)
constexpr int A1P_WROWS = A1P_MAXCH * 32 + 32;                          // 320 window rows
constexpr int A1P_OROW = DH + 8;                                        // output stage row (bf16): 144 B
constexpr size_t A1P_KS = (size_t)NL * Lay<bf16>::KROW * 2;             // 36864
constexpr size_t A1P_VT = (size_t)NL * Lay<bf16>::VROW * 2;             // 40960
constexpr size_t A1P_WIN = (size_t)A1P_WROWS * DH * 2;                  // 40960
constexpr size_t A1P_OST = (size_t)32 * A1P_OROW * 2;                   // 4608 per wave
constexpr size_t A1P_WIN_OFF = A1P_KS + A1P_VT;
constexpr size_t A1P_OST_OFF = A1P_WIN_OFF + A1P_WIN;
constexpr size_t A1P_BAND_OFF = A1P_OST_OFF + A1P_WAVES * A1P_OST;      // [4][64] x 16 B
constexpr size_t A1P_TAPS_OFF = A1P_BAND_OFF + 4 * 64 * 16;
constexpr size_t A1P_BYTES = A1P_TAPS_OFF + 128 * sizeof(float);        // 162304

// diagnostic stamps (STAMP instantiations only): [block][wave][slot] s_memtime, read by tm_debug_a1_stamps
__device__ unsigned long long g_a1_stamps[512 * 8 * 8];
template <bool STAMP>
TM_DEV void a1p_stamp(int slot, int wave) {
  if constexpr (STAMP) {
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0)
      g_a1_stamps[((blockIdx.y * gridDim.x + blockIdx.x) * 8 + wave) * 8 + slot] = t;
  }
}

TM_DEV void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// A operand of the conv product: window rows kb.. (acc_k_index order, as value_frag)
TM_DEV bf16x8 a1p_window_frag(const bf16* win, int dt, int kb, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int d = dt * 32 + (g & 1) * 16 + 4 * p;
  const int key = kb + 4 * (g >> 1) + q;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(win + key * DH + d));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(win + (key + 8) * DH + d));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// attn_fwd_wave with the per-tile work interleaved for the scheduler (the max tree of score tile
// kt beside the MFMAs of tile kt + 1, the exp / sum / bf16 packing of tile kt beside its P.V
// MFMAs) and its LDS fragments software-pipelined one tile ahead: one wave per SIMD has no
// partner wave to hide a read's latency.  Key fragments of tile kt + 1 and value fragments of
// tile kt + 1 are issued before the MFMAs of tile kt; the max tree of tile kt - 1 and the exp /
// pack of tile kt + 1 run beside them.  Same arithmetic and order of every sum as the form with
// just-in-time reads it replaced (bitwise equal; 14.4 -> 13.8 us per call at the bench shape).
TM_DEV void attn_fwd_wave_pipe(const bf16* ks, const bf16* vt, const bf16x8 (&qf)[4], f32x16 (&o)[2], float& mx,
                               float& sum, int lane) {
  constexpr int KROW = Lay<bf16>::KROW;
  const int r = lane & 31, h = lane >> 5;
  f32x16 s[8];
  float mk[8];
  bf16x8 kf[2][4];
#pragma unroll
  for (int st = 0; st < 4; ++st) kf[0][st] = load8(ks + r * KROW + st * 16 + 8 * h);
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    if (kt < 7) {
#pragma unroll
      for (int st = 0; st < 4; ++st) kf[(kt + 1) & 1][st] = load8(ks + ((kt + 1) * 32 + r) * KROW + st * 16 + 8 * h);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead (the scheduler sinks reads to their use)
    s[kt] = (f32x16){};
#pragma unroll
    for (int st = 0; st < 4; ++st) mma16(s[kt], kf[kt & 1][st], qf[st]);
    if (kt > 0) mk[kt - 1] = tree_max16(s[kt - 1]);
    __builtin_amdgcn_sched_barrier(0);
  }
  mk[7] = tree_max16(s[7]);
  float m = fmaxf(fmaxf(fmaxf(mk[0], mk[1]), fmaxf(mk[2], mk[3])), fmaxf(fmaxf(mk[4], mk[5]), fmaxf(mk[6], mk[7])));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float ml = m * LOG2E;
  o[0] = (f32x16){};
  o[1] = (f32x16){};
  float lk[8];
  bf16x8 vf[2][4], pf[2][2];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) vf[0][2 * sp + dt] = value_frag<bf16>(vt, dt, 16 * sp, lane);
#pragma unroll
  for (int i = 0; i < 16; ++i) s[0][i] = __builtin_amdgcn_exp2f(fmaf(s[0][i], LOG2E, -ml));
  lk[0] = tree_sum16(s[0]);
  pf[0][0] = acc_as_operand<bf16>(s[0], 0);
  pf[0][1] = acc_as_operand<bf16>(s[0], 1);
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const int b = kt & 1, nb = b ^ 1;
    if (kt < 7) {
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) vf[nb][2 * sp + dt] = value_frag<bf16>(vt, dt, (kt + 1) * 32 + 16 * sp, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) mma16(o[dt], vf[b][2 * sp + dt], pf[b][sp]);
    if (kt < 7) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kt + 1][i] = __builtin_amdgcn_exp2f(fmaf(s[kt + 1][i], LOG2E, -ml));
      lk[kt + 1] = tree_sum16(s[kt + 1]);
      pf[nb][0] = acc_as_operand<bf16>(s[kt + 1], 0);
      pf[nb][1] = acc_as_operand<bf16>(s[kt + 1], 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  float l = ((lk[0] + lk[1]) + (lk[2] + lk[3])) + ((lk[4] + lk[5]) + (lk[6] + lk[7]));
  l += __shfl_xor(l, 32, 64);
  mx = m;
  sum = l;
}

template <bool STAMP = false>   // STAMP: per-wave s_memtime stamps (diagnostic build only)
__global__ __launch_bounds__(256) void a1_fwd_bf16_kernel(const bf16* __restrict__ q, const bf16* __restrict__ v,
                                                          const bf16* __restrict__ kl_t, const bf16* __restrict__ y_t,
                                                          const float* __restrict__ wconv, int n, int nh, int wpg,
                                                          bf16* __restrict__ merged, float* __restrict__ lse1) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* ks = (bf16*)smem;
  bf16* vt = (bf16*)(smem + A1P_KS);
  bf16* win = (bf16*)(smem + A1P_WIN_OFF);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  bf16* ost = (bf16*)(smem + A1P_OST_OFF + wave * A1P_OST);
  bf16x8* band_tab = (bf16x8*)(smem + A1P_BAND_OFF);
  float* taps = (float*)(smem + A1P_TAPS_OFF);
  const int bh = blockIdx.y, gi = blockIdx.x;
  const int head = bh % nh, bag = bh / nh;
  const int cph = n / 32;                          // 32-query chunks of this head
  const int c_begin = (int)((long long)gi * cph / wpg), c_end = (int)((long long)(gi + 1) * cph / wpg);
  const int w0 = c_begin * 32 - HALF;              // sequence row of window row 0
  const int wrows = (c_end - c_begin) * 32 + 2 * HALF;
  const bf16* qb = q + (size_t)bh * n * DH;
  const bf16* vb = v + (size_t)bh * n * DH;
  const int ld = nh * DH;
  a1p_stamp<STAMP>(0, wave);

  // ---- prologue: keys, Y, taps and this wave's first query fragments through registers;
  //      the v window by LDS-DMA, left in flight through the first attention phase ----
  int c = c_begin + wave;
  bf16x8 qf[4];
  if (c < c_end) {
#pragma unroll
    for (int st = 0; st < 4; ++st) qf[st] = load8(qb + (size_t)(c * 32 + r) * DH + st * 16 + 8 * h);
  }
  TileRegs<bf16, 256> kr, yr;
  kr.load(kl_t + (size_t)bh * NL * DH, tid);
  yr.load(y_t + (size_t)bh * NL * DH, tid);
  float tapv = 0.f;
  if (tid < 128) {
    const int tau = tid - 32;  // taps[k] = w[k - 32], zero outside the filter
    if (tau >= 0 && tau < TAPS) tapv = wconv[head * TAPS + tau];
  }
  {
    typedef __attribute__((address_space(3))) void lds_t;
    typedef __attribute__((address_space(1))) void glb_t;
#pragma unroll
    for (int i = 0; i < A1P_WROWS * 8 / 256; ++i) {
      const int pc = i * 256 + tid, row = pc >> 3;  // 16-B piece pc of the window image
      if (i * 32 < wrows) {                         // wave-uniform: 8 rows per wave-instruction
        const int src = min(max(w0 + row, 0), n - 1);
        __builtin_amdgcn_global_load_lds((glb_t*)(vb + (size_t)src * DH + (pc & 7) * 8),
                                         (lds_t*)(win + (size_t)(i * 256 + wave * 64) * 8), 16, 0, 0);
      }
    }
  }
  kr.store_keys(ks, tid);
  yr.store_values(vt, tid);
  if (tid < 128) taps[tid] = tapv;
  __syncthreads();  // taps visible
  {  // interior band fragments: element jj of lane (rr, hh), k-step s = wave
    const int s = tid >> 6, ln = tid & 63, rr = ln & 31, hh = ln >> 5;
    bf16x8 b;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) b[jj] = (bf16)taps[16 * s + 8 * (jj >> 2) + 4 * hh + (jj & 3) - rr + 32];
    band_tab[s * 64 + ln] = b;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // keys / Y / band table in LDS; the window DMA may still be in flight
  a1p_stamp<STAMP>(1, wave);

  bool first = true;
  for (;;) {
    const bool active = c < c_end;
    const int t0 = c * 32;
    f32x16 o[2];
    float mx = 0.f, sum = 1.f;
    if (active) attn_fwd_wave_pipe(ks, vt, qf, o, mx, sum, lane);
    if (first) a1p_stamp<STAMP>(2, wave);
    const int cn = c + A1P_WAVES;
    if (cn < c_end) {
#pragma unroll
      for (int st = 0; st < 4; ++st) qf[st] = load8(qb + (size_t)(cn * 32 + r) * DH + st * 16 + 8 * h);
    }
    if (first) {
      // every wave's window pieces have landed (the next chunk's 4 query loads may not)
      if (cn < c_end) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      first = false;
      a1p_stamp<STAMP>(3, wave);
    }
    if (!active) break;
    // band fragments from the shared table.  At the sequence ends the window rows outside
    // [0, n) are exactly one k-step: rows j < 16 (k-step 0) for t0 = 0, rows j >= 48 (k-step 3)
    // for the last chunk -- those fragments are zeroed.
    bf16x8 band[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) band[s] = band_tab[s * 64 + lane];
    if (t0 == 0) band[0] = bf16x8{};
    if (t0 + 32 == n) band[3] = bf16x8{};
    const float inv = 1.0f / sum;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[dt][i] *= inv;
    const bf16* wc = win + (size_t)(t0 - HALF - w0) * DH;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int s = 0; s < 4; ++s) mma16(o[dt], a1p_window_frag(wc, dt, 16 * s, lane), band[s]);
    if (c == c_begin + wave) a1p_stamp<STAMP>(4, wave);
    if (h == 0) lse1[(size_t)bh * n + t0 + r] = mx + __logf(sum);
    // O^T registers -> [32 q][72] bf16 wave stage -> full 128-B row stores, 16 B per lane
    // (row-per-lane 8-B stores are store-issue bound)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = (bf16)o[dt][4 * g4 + e];
        *(bf16x4*)(ost + r * A1P_OROW + dt * 32 + 8 * g4 + 4 * h) = pk;
      }
    wave_lds_fence();
    f32x4 ov[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = lane + 64 * i;
      ov[i] = *(const f32x4*)(ost + (p >> 3) * A1P_OROW + (p & 7) * 8);
    }
    bf16* dst = merged + ((size_t)bag * n + t0) * ld + head * DH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = lane + 64 * i;
      *(f32x4*)(dst + (size_t)(p >> 3) * ld + (p & 7) * 8) = ov[i];
    }
    wave_lds_fence();  // stage read back before the next chunk rewrites it
    if (c == c_begin + wave) a1p_stamp<STAMP>(5, wave);
    c = cn;
    if (c >= c_end) break;
  }
  a1p_stamp<STAMP>(6, wave);
}

// A3 path forward, bf16 (bench mode): one 512-thread workgroup per CU holds ALL 256 landmark
// queries of its head (8 waves x 32) against an even share of the head's keys, so k and v are read
// from HBM once (the 128-query form read them twice) and a head has P (<= 32) partials instead of
// 2 x n/256 half-slabs.  grid (P, nbh); workgroup p takes the 32-key sub-blocks
// [p S32 / P, (p + 1) S32 / P) (S32 = n / 32) in chunks of up to A3V_G sub-blocks, double-buffered
// in LDS (k [key][72], v [key][80]): the next chunk's 16-B pieces are requested into registers before
// the current chunk's scores, so its HBM round trip overlaps them; online softmax across chunks.
//   part_o[p][bh][q][d] = sum_keys exp(s - m) v ; part_m, part_l[p][bh][q] = (m, l)
constexpr int A3V_G = 5;                                           // sub-blocks (32 keys) per chunk
constexpr int A3V_KEYS = A3V_G * 32;
constexpr size_t A3V_KS = (size_t)A3V_KEYS * Lay<bf16>::KROW * 2;  // 23040 B
constexpr size_t A3V_BUF = A3V_KS + (size_t)A3V_KEYS * Lay<bf16>::VROW * 2;   // + 25600 B
constexpr size_t A3V_BYTES = 2 * A3V_BUF;                          // two chunk buffers: 97280 B
constexpr int A3V_PIECES = (A3V_KEYS * 8 + 511) / 512;             // 16-B pieces per thread per operand

// partials per head of the v2 kernel
inline int a3v_splits(int nbh, int n) { return std::max(1, std::min(n / 32, tm_cu_count() / std::max(nbh, 1))); }

// S2R > 0: the workgroup also writes A2 = softmax(q~ k~^T) rows p * 2 S2R .. + 2 S2R - 1 of its head
// (sim2_wave_rows, rows dealt over the 8 waves; host-checked 2 S2R P == 256) before its first key
// chunk is staged: the k~ / q~ loads go out ahead of the chunk's, so the rows are computed while the
// chunk is in flight, and the separate sim2 launch disappears from the step.
struct Sim2Out { const float* kl; float* a2; bf16* a2s; };
template <int ST = 0, int S2R = 0>   // ST: diagnostic s_memtime stamps (g_a1_stamps)
__global__ __launch_bounds__(512) void a3_fwd_v2_kernel(const float* __restrict__ ql, const bf16* __restrict__ k,
                                                        const bf16* __restrict__ v, int n, int P,
                                                        bf16* __restrict__ part_o, float* __restrict__ part_m,
                                                        float* __restrict__ part_l, Sim2Out s2) {
  constexpr int KROW = Lay<bf16>::KROW, VROW = Lay<bf16>::VROW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x, bh = blockIdx.y, nbh = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  auto stamp = [&](int slot) { if (ST) a1p_stamp<ST != 0>(slot, wave); };
  stamp(0);
  const int S32 = n / 32;
  const int sb0 = (int)((long long)p * S32 / P), sb1 = (int)((long long)(p + 1) * S32 / P);
  const int qi = wave * 32 + r;
  const bf16* kh = k + (size_t)bh * n * DH;
  const bf16* vh = v + (size_t)bh * n * DH;
  f32x4 kr[A3V_PIECES], vr[A3V_PIECES];
  // the 16-B pieces of the chunk starting at sub-block c0 (rows clamped into the chunk)
  auto fetch = [&](int c0) {
    const int rows = min(A3V_G, sb1 - c0) * 32;
#pragma unroll
    for (int j = 0; j < A3V_PIECES; ++j) {
      const int i = tid + 512 * j, row = min(i >> 3, rows - 1), c = (i & 7) * 8;
      const size_t o = ((size_t)c0 * 32 + row) * DH + c;
      kr[j] = *(const f32x4*)(kh + o);
      vr[j] = *(const f32x4*)(vh + o);
    }
  };
  auto stage = [&](int c0, int buf) {
    const int rows = min(A3V_G, sb1 - c0) * 32;
    bf16* ks = (bf16*)(smem + buf * A3V_BUF);
    bf16* vs = (bf16*)(smem + buf * A3V_BUF + A3V_KS);
#pragma unroll
    for (int j = 0; j < A3V_PIECES; ++j) {
      const int i = tid + 512 * j, row = i >> 3, c = (i & 7) * 8;
      if (row < rows) {
        *(f32x4*)(ks + row * KROW + c) = kr[j];
        *(f32x4*)(vs + row * VROW + c) = vr[j];
      }
    }
  };
  // fused A2 rows (S2R > 0): computed AFTER the key loop, from k~ loaded into registers during the
  // first key chunk (so its L2 round trip hides under the chunk's MFMAs) and written into the LDS the
  // chunk buffers leave free; the A2 rows then cost only the tail's LDS staging and arithmetic (the
  // prologue form made the first key chunk wait for them: +5 us per call)
  constexpr int S2Q = S2R > 0 ? S2R * DH / 256 : 1;
  float q2[S2Q];
  f32x4 k2[S2R > 0 ? 8 : 1];
  const int g2 = tid >> 8, j2 = tid & 255, r2 = p * 2 * S2R + g2 * S2R;
  fetch(sb0);
  if constexpr (S2R > 0) {
#pragma unroll
    for (int u = 0; u < S2Q; ++u) q2[u] = ql[((size_t)bh * NL + r2) * DH + u * 256 + j2];
  }
  bf16x8 qf[4];
#pragma unroll
  for (int st = 0; st < 4; ++st) qf[st] = cvt8<bf16>(ql + ((size_t)bh * NL + qi) * DH + st * 16 + 8 * h);
  stamp(1);
  stage(sb0, 0);
  __syncthreads();
  stamp(2);
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o[2];
  o[0] = (f32x16){};
  o[1] = (f32x16){};
  int buf = 0;
  for (int c0 = sb0; c0 < sb1; c0 += A3V_G) {
    const int ng = min(A3V_G, sb1 - c0);
    const bool more = c0 + A3V_G < sb1;
    if (more) fetch(c0 + A3V_G);   // in flight through this chunk's scores
    if constexpr (S2R > 0) {
      if (c0 == sb0) {   // k~ of the head for the A2 rows of the tail (16-B pieces: row p / 16, d 4 (p % 16))
        const float* kb = s2.kl + (size_t)bh * NL * DH;
#pragma unroll
        for (int u = 0; u < 8; ++u) k2[u] = *(const f32x4*)(kb + (size_t)(u * 512 + tid) * 4);
      }
    }
    const bf16* ks = (const bf16*)(smem + buf * A3V_BUF);
    const bf16* vs = (const bf16*)(smem + buf * A3V_BUF + A3V_KS);
    f32x16 s[A3V_G];   // S^T tiles (rows = keys, col = this lane's query)
#pragma unroll
    for (int kt = 0; kt < A3V_G; ++kt) {
      s[kt] = (f32x16){};
      if (kt < ng) {
#pragma unroll
        for (int st = 0; st < 4; ++st) mma16(s[kt], load8(ks + (kt * 32 + r) * KROW + st * 16 + 8 * h), qf[st]);
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < A3V_G; ++kt)
      if (kt < ng) m = fmaxf(m, tree_max16(s[kt]));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float m_new = fmaxf(m_run, m);
    const float corr = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);   // 0 on the first chunk
    const float ml = m_new * LOG2E;
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < A3V_G; ++kt) {
      if (kt < ng) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kt][i] = __builtin_amdgcn_exp2f(fmaf(s[kt][i], LOG2E, -ml));
        l += tree_sum16(s[kt]);
      }
    }
    l += __shfl_xor(l, 32, 64);
    l_run = l_run * corr + l;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      o[dt] *= corr;
#pragma unroll
      for (int kt = 0; kt < A3V_G; ++kt)
        if (kt < ng) {
#pragma unroll
          for (int sp = 0; sp < 2; ++sp)
            mma16(o[dt], value_frag<bf16>(vs, dt, kt * 32 + 16 * sp, lane), acc_as_operand<bf16>(s[kt], sp));
        }
    }
    if (c0 == sb0) stamp(3);
    if (more) {
      stage(c0 + A3V_G, buf ^ 1);   // the other buffer: last read two chunks ago, before the barrier below
      __syncthreads();
      buf ^= 1;
    }
    if (c0 == sb0) stamp(4);
  }
  stamp(5);
  if constexpr (S2R > 0) {
    // (before the partial stores: a barrier behind them would wait for their write-back)
    __syncthreads();   // every wave is done with the chunk buffers
    float* kimg = (float*)smem;                        // k~ row image [256][64]: row j's chunk c at slot c ^ (j & 15)
    float* qs = kimg + S2_KIMG + g2 * S2R * DH;        // [2 S2R rows][64]: group g2's rows at g2 S2R
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int pc = u * 512 + tid, row = pc >> 4, c = pc & 15;
      *(f32x4*)(kimg + row * DH + ((c ^ (row & 15)) << 2)) = k2[u];
    }
#pragma unroll
    for (int u = 0; u < S2Q; ++u) qs[u * 256 + j2] = q2[u];
    __syncthreads();
    stamp(7);          // (diagnostic: k~ staged)
    // wave w: A2 rows p 2 S2R + w + 8 k, k < 2 S2R / 8 (the 8 waves split the 2 S2R rows evenly)
    constexpr int RW = S2R > 0 ? 2 * S2R / 8 : 1;
    static_assert(S2R == 0 || (2 * S2R) % 8 == 0, "fused A2 rows: a multiple of 8 rows per workgroup");
    sim2_wave_rows<RW>(kimg, kimg + S2_KIMG, wave, 8, lane, s2.a2, s2.a2s,
                       ((size_t)bh * NL + (size_t)p * 2 * S2R + wave) * NL, (size_t)8 * NL, (size_t)nbh * NL * NL);
  }
  const size_t pidx = ((size_t)p * nbh + bh) * NL + qi;
  if (h == 0) { part_m[pidx] = m_run; part_l[pidx] = l_run; }
  // the unnormalised partial sum in bf16 (half the slab bytes out and through the combine, which
  // merges the partials in fp32); m / l stay fp32
  bf16* po = part_o + pidx * DH;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      *(bf16x4*)(po + dt * 32 + 8 * g4 + 4 * h) =
          (bf16x4){(bf16)o[dt][4 * g4], (bf16)o[dt][4 * g4 + 1], (bf16)o[dt][4 * g4 + 2], (bf16)o[dt][4 * g4 + 3]};
  if (ST) {
    __builtin_amdgcn_s_waitcnt(0);
    stamp(6);
  }
}

// combine of the v2 partials: grid (nbh, 32), block 256 (a3_combine.h; the bench step runs the same
// routine inside the pseudo-inverse chain's last launch instead, tm_pinv_fwd_split_a3)
__global__ __launch_bounds__(256) void a3_combine_v2_kernel(A3Combine c) {
  __shared__ A3CombineLds lds;
  const A3CombineState st = a3_combine_phase1(c, blockIdx.x, blockIdx.y, threadIdx.x, lds, true);
  __syncthreads();
  a3_combine_phase2(c, blockIdx.x, blockIdx.y, threadIdx.x, lds, st, true);
}

// ---------------------------------------------------------------------------
// bf16 conv33 backward on the MFMA.  One workgroup = one head x R rows, R = n * nbh / 256
// rounded up to 8 (<= 288): 256 workgroups at N = 8192 (the fp32-LDS kernel of nystrom_f32.h runs 1056
// workgroups of 64 rows, three rounds deep, bound by its LDS reads: 30 us).  Windows of 320
// rows (t0 - 16 ..) of dO and v as bf16 row-major LDS images; per 32-row tile i (wave w takes
// tiles w, w + 8):
//   S  = dO[tile] v_win[32i .. 32i + 63]^T (2 MFMA tiles, K = 64)  ->  c_tau(t) = S[r][r + tau]
//   dv = Toep(w) dO_win[32i .. 32i + 63],  Toep[r][k] = w[r + 32 - k]  (w as bf16 hi + lo, so
//        the taps keep ~16 bits; the products of bf16 operands are exact in the fp32 sums)
constexpr int CB_ROWS = 288, CB_WIN = CB_ROWS + 2 * HALF, CB_ROW = DH + 8, CB_ST = 66;
struct CbLay {
  static constexpr size_t DO_OFF = 0;
  static constexpr size_t V_OFF = DO_OFF + (size_t)CB_WIN * CB_ROW * 2;
  static constexpr size_t ST_OFF = V_OFF + (size_t)CB_WIN * CB_ROW * 2;  // [8 waves][32][66] fp32
  static constexpr size_t W_OFF = ST_OFF + 8 * 32 * CB_ST * 4;            // taps fp32
  static constexpr size_t CS_OFF = W_OFF + 64 * 4;                        // [8 waves][36] tap sums
  static constexpr size_t BYTES = CS_OFF + 8 * 36 * 4;                    // 161152
};

// rows per workgroup of the bf16 conv backward (one workgroup per CU over all heads when possible)
inline int conv_bwd_rows(int nbh, int n) {
  const long long cu = tm_cu_count();
  const long long want = ((long long)n * nbh + cu - 1) / cu;
  const int r = (int)((want + 7) / 8 * 8);
  return r < 32 ? 32 : (r > CB_ROWS ? CB_ROWS : r);
}

// standard B fragment (lane: col = mb + (lane & 31), k = kb + 8 (lane >> 5) + j) of a row-major
// [k][ldr] bf16 LDS image, by two transposing reads
TM_DEV bf16x8 frag_tr_rows(const bf16* S, int ldr, int mb, int kb, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int m = mb + (g & 1) * 16 + 4 * p;
  const int k = kb + 8 * (g >> 1) + q;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(S + k * ldr + m));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(S + (k + 4) * ldr + m));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__global__ __launch_bounds__(512) void conv_bwd_mfma_kernel(const bf16* __restrict__ dmerged,
                                                            const bf16* __restrict__ merged,
                                                            const bf16* __restrict__ v,
                                                            const float* __restrict__ wconv, int n, int nh, int R,
                                                            bf16* __restrict__ dv, float* __restrict__ d1,
                                                            float* __restrict__ dw_part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* dos = (bf16*)(smem + CbLay::DO_OFF);
  bf16* vws = (bf16*)(smem + CbLay::V_OFF);
  float* ws = (float*)(smem + CbLay::W_OFF);
  float* csum = (float*)(smem + CbLay::CS_OFF);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int head = bh % nh, bag = bh / nh, ld = nh * DH;
  const int t0 = blk * R;
  const int rows = min(R, n - t0);
  const bf16* dob = dmerged + (size_t)bag * n * ld + head * DH;
  const bf16* ob = merged + (size_t)bag * n * ld + head * DH;
  const bf16* vb = v + (size_t)bh * n * DH;
  // the two windows in one burst (rows past what the block's tiles read stay zero)
  constexpr int PW = CB_WIN * 8 / 512;
  bf16x8 ca[PW], cb[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int i = tid + 512 * j, w = i >> 3, d0 = (i & 7) * 8, t = t0 - HALF + w;
    const bool ok = t >= 0 && t < n && w < rows + 2 * HALF;
    const int tc = ok ? t : 0;
    ca[j] = load8(dob + (size_t)tc * ld + d0);
    cb[j] = load8(vb + (size_t)tc * DH + d0);
    if (!ok) { ca[j] = (bf16x8){}; cb[j] = (bf16x8){}; }
  }
  if (tid < TAPS) ws[tid] = wconv[head * TAPS + tid];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int i = tid + 512 * j, w = i >> 3, d0 = (i & 7) * 8;
    *(bf16x8*)(dos + w * CB_ROW + d0) = ca[j];
    *(bf16x8*)(vws + w * CB_ROW + d0) = cb[j];
  }
  __syncthreads();
  // Toeplitz A fragments (the same for every tile): lane row r32, k = 16 s + 8 h + j
  bf16x8 th[4], tl[4];
#pragma unroll
  for (int st = 0; st < 4; ++st) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int tau = r32 + 32 - (16 * st + 8 * h + j);
      const float wv = (tau >= 0 && tau < TAPS) ? ws[tau] : 0.f;
      const bf16 hi = (bf16)wv;
      th[st][j] = hi;
      tl[st][j] = (bf16)(wv - (float)hi);
    }
  }
  float* stg = (float*)(smem + CbLay::ST_OFF) + wave * 32 * CB_ST;
  constexpr int NTK = (TAPS + 1) / 2;  // taps per lane: tau = h + 2k (17)
  float csl[NTK];
#pragma unroll
  for (int k = 0; k < NTK; ++k) csl[k] = 0.f;
  const int ntile = (rows + 31) / 32;
#pragma unroll 1
  for (int i = wave; i < ntile; i += 8) {
    // S = dO[tile] . v_win[32i .. 32i + 63]^T
    f32x16 sa = (f32x16){}, sb = (f32x16){};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const bf16x8 a = *(const bf16x8*)(dos + (32 * i + HALF + r32) * CB_ROW + 16 * st + 8 * h);
      const bf16x8 ba = *(const bf16x8*)(vws + (32 * i + r32) * CB_ROW + 16 * st + 8 * h);
      const bf16x8 bb = *(const bf16x8*)(vws + (32 * i + 32 + r32) * CB_ROW + 16 * st + 8 * h);
      mma16(sa, a, ba);
      mma16(sb, a, bb);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = acc_row(reg, h);
      stg[row * CB_ST + r32] = sa[reg];
      stg[row * CB_ST + 32 + r32] = sb[reg];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // band: lane (row r32, taps h + 2k); the row's dO . O over d 32h .. 32h + 31
    const int lr = 32 * i + r32;
    const bool rv = lr < rows;
    float wc = 0.f, dd = 0.f;
#pragma unroll
    for (int k = 0; k < NTK; ++k) {
      const int tau = h + 2 * k;
      if (tau < TAPS) {
        const float c = stg[r32 * CB_ST + r32 + tau];
        if (rv) { csl[k] += c; wc = fmaf(ws[tau], c, wc); }
      }
    }
    if (rv) {
      const bf16* orow = ob + (size_t)(t0 + lr) * ld + 32 * h;
      const bf16* grow = dos + (lr + HALF) * CB_ROW + 32 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bf16x8 o8 = load8(orow + 8 * q), g8 = *(const bf16x8*)(grow + 8 * q);
#pragma unroll
        for (int e = 0; e < 8; ++e) dd = fmaf((float)g8[e], (float)o8[e], dd);
      }
    }
    float tot = dd - wc;
    tot += __shfl_xor(tot, 32, 64);
    if (rv && h == 0) d1[(size_t)bh * n + t0 + lr] = tot;
    // dv tile = Toep . dO_win[32i .. 32i + 63]
    const bf16* dwin = dos + 32 * i * CB_ROW;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      f32x16 acc = (f32x16){};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const bf16x8 b = frag_tr_rows(dwin, CB_ROW, dt * 32, 16 * st, lane);
        mma16(acc, th[st], b);
        mma16(acc, tl[st], b);
      }
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int l2 = 32 * i + acc_row(reg, h);
        if (l2 < rows) dv[((size_t)bh * n + t0 + l2) * DH + dt * 32 + r32] = (bf16)acc[reg];   // bf16: read once by the fused A3 backward
      }
    }
    __builtin_amdgcn_wave_barrier();   // the stage is rewritten by the wave's next tile
  }
  // tap sums: over the 32 rows of each lane half, then over the waves in a fixed order
#pragma unroll
  for (int k = 0; k < NTK; ++k) {
    float x = csl[k];
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o, 64);
    const int tau = h + 2 * k;
    if (r32 == 0 && tau < TAPS) csum[wave * 36 + tau] = x;
  }
  __syncthreads();
  if (tid < TAPS) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += csum[w * 36 + tid];
    dw_part[((size_t)bag * nblk + blk) * (nh * TAPS) + head * TAPS + tid] = sum;
  }
}

// Selectors of the diagnostic build (tm_debug_set_nys_sel; NYS_SEL in scripts/microbench.py): the
// stamped instantiations of the shipped bf16 kernels (per-wave s_memtime into g_a1_stamps; the
// _CHUNK forms stamp inside one query chunk instead of the phases).  The product compiles NYS_AUTO in.
enum NysSel { NYS_AUTO = 0, NYS_STAMP_A1_FWD, NYS_STAMP_A3_FWD, NYS_STAMP_A1_BWD, NYS_STAMP_A1_BWD_CHUNK,
              NYS_STAMP_A3_BWD, NYS_STAMP_A3_BWD_CHUNK };
#ifdef TM_DIAG
int g_nys_sel = NYS_AUTO;
#endif
#define NYS_SEL TM_DIAG_VAR(g_nys_sel)

// ---------------------------------------------------------------------------
// bf16 attention backward with every operand of the workgroup staged ONCE: the
// workgroup's <= 256 query rows of Q and dO ([q][72] row-major images), their lse / D,
// K^T and the wave's K / V fragments are all requested in one burst before the query
// walk, so the walk itself issues no global loads (the per-chunk version paid two
// dependent HBM round trips per 32-query chunk).  dV/dK operands come from the same
// row-major images through transposing reads (acc_as_operand k order).
// NW waves = NW 32-key units per workgroup; MQ = staged query rows.  <8, 288>: A1 (the 256
// landmark keys, <= 9 query chunks) and the A3 key blocks of 256; <9, 256>: A3 with the n / 32 key
// units of a head split evenly over 256 / nbh workgroups (8-9 units each: one chip round at
// N = 8192 where 33 blocks of 256 keys per head were 264 workgroups on 256 CUs).
template <int NW, int MQ>
struct BwdLayT {
  static constexpr int MAXQ = MQ;
  static constexpr int NK = 32 * NW;  // key columns
  static constexpr int KT_ROW = NK + 8, DS_ROW = NK + 8, QROW = DH + 8;
  static constexpr size_t KT_OFF = 0;
  static constexpr size_t DS_OFF = KT_OFF + DH * KT_ROW * 2;
  static constexpr size_t QS_OFF = DS_OFF + 32 * DS_ROW * 2;
  static constexpr size_t OS_OFF = QS_OFF + MAXQ * QROW * 2;
  static constexpr size_t XC_OFF = OS_OFF + MAXQ * QROW * 2;  // fp32 [3][32 q][64 d] key-group dq partials
  static constexpr size_t LS_OFF = XC_OFF + 6 * 1024 * 4;     // fp32 lse[MAXQ], D[MAXQ]
  static constexpr size_t MAIN = LS_OFF + 2 * MAXQ * 4;       // 160512 B (<8, 288>), 157184 B (<9, 256>)
  static constexpr size_t EPI = (size_t)NK * 68 * 4;
  static constexpr size_t BYTES = MAIN > EPI ? MAIN : EPI;
};
using BwdLay16 = BwdLayT<8, 288>;
using BwdLay9 = BwdLayT<9, 256>;
static_assert(BwdLay9::BYTES <= 160 * 1024 && BwdLay16::BYTES <= 160 * 1024, "bf16 backward layout exceeds the CU's LDS");

// A-operand fragment (rows m = mb + l32, 8 k in acc_as_operand order) of a row-major
// [k][QROW] bf16 image: element j of lane half h <-> k = kb + 8 (j >> 2) + 4 h + (j & 3)
template <int R>
TM_DEV bf16x8 frag_tr_rows(const bf16* S, int mb, int kb, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int m = mb + (g & 1) * 16 + 4 * p;
  const int k = kb + 4 * (g >> 1) + q;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(S + k * R + m));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(S + (k + 8) * R + m));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
TM_DEV bf16x8 frag_tr_acc(const bf16* S, int mb, int kb, int lane) { return frag_tr_rows<BwdLay16::QROW>(S, mb, kb, lane); }

// dQ = dS K by two waves, one 32-column d tile each over ALL the workgroup's keys in one
// accumulation chain (no cross-wave partials through LDS, no third barrier per chunk; the other
// waves go on to the next chunk's S / dP / dV / dK meanwhile).
template <int MODE, int NW = 8, int ST = 0>   // ST: diagnostic s_memtime stamps (g_a1_stamps): 1 phases, 2 one chunk
__global__ __launch_bounds__(64 * NW) void attn_bwd_bf16_kernel(BwdArgs a) {
  using LY = std::conditional_t<NW == 9, BwdLay9, BwdLay16>;
  static_assert(NW == 8 || (NW == 9 && MODE == MODE_A3), "9-wave form: A3 even split only");
  constexpr int NT = 64 * NW;
  constexpr int KT_ROW = LY::KT_ROW, DS_ROW = LY::DS_ROW, QROW = LY::QROW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* kt_s = (bf16*)(smem + LY::KT_OFF);
  bf16* ds_s = (bf16*)(smem + LY::DS_OFF);
  bf16* qs = (bf16*)(smem + LY::QS_OFF);
  bf16* os = (bf16*)(smem + LY::OS_OFF);
  float* lse_s = (float*)(smem + LY::LS_OFF);
  float* dd_s = lse_s + LY::MAXQ;
  float* stage = (float*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int blk = blockIdx.x, bh = blockIdx.y, nh = a.nh;
  auto stamp = [&](int slot) { if (ST == 1 && wave < 8) a1p_stamp<ST != 0>(slot, wave); };
  auto cstamp = [&](int c0, int slot) { if (ST == 2 && c0 == 64 && wave < 8) a1p_stamp<ST != 0>(slot, wave); };
  stamp(0);
  int key0 = (MODE == MODE_A3) ? blk * NL : 0;
  int nunits = 8;  // 32-key units of this workgroup (wave w < nunits owns keys key0 + 32 w ..)
  if (MODE == MODE_A3 && a.q_total > 0) {
    // even split of the head's n / 32 key units over the gridDim.x workgroups (<= NW each, host-checked)
    const int upk = a.n_key_rows / 32;
    const int u0 = (int)((long long)blk * upk / gridDim.x), u1 = (int)((long long)(blk + 1) * upk / gridDim.x);
    key0 = 32 * u0;
    nunits = u1 - u0;
  }
  const int nk = 32 * nunits;
  const bool active = wave < nunits;
  int q_begin = (MODE == MODE_A1) ? blk * a.n_queries_per_wg : 0;
  int q_count = a.n_queries_per_wg;  // <= 256, a multiple of 32 (host-checked)
  if (MODE == MODE_A1 && a.q_total > 0) {
    // even split of the q_total / 32 query chunks over the gridDim.x workgroups of a head: at
    // N = 8192 that is 8-9 chunks for each of 32 workgroups (256 = one per CU) instead of 33
    // blocks of 8 chunks (264 > 256 CUs: a second round for 8 of them)
    const int cph = a.q_total / 32;
    const int c0 = (int)((long long)blk * cph / gridDim.x), c1 = (int)((long long)(blk + 1) * cph / gridDim.x);
    q_begin = 32 * c0;
    q_count = 32 * (c1 - c0);  // <= MAXQ (host-checked)
  }

  const bf16* Q = (const bf16*)a.q + hoff(bh, nh, a.q_bag, a.q_head) + (size_t)q_begin * a.q_row;
  const bf16* dO = (const bf16*)a.dO + hoff(bh, nh, a.o_bag, a.o_head) + (size_t)q_begin * a.o_row;
  const bf16* K = (const bf16*)a.k + hoff(bh, nh, a.k_bag, a.k_head) + (size_t)key0 * DH;
  const bf16* V = (const bf16*)a.v + hoff(bh, nh, a.v_bag, a.v_head) + (size_t)key0 * DH;
  const float* lse = a.lse + bh * a.lse_bh + q_begin;
  const float* dd = a.dd + bh * a.dd_bh + q_begin;
  const float* dd2 = a.dd2 ? a.dd2 + bh * a.dd_bh + q_begin : nullptr;

  // ---- one burst of loads: K rows (for K^T), Q / dO rows, K / V fragments, lse / D ----
  constexpr int QP = (LY::MAXQ * 8 + NT - 1) / NT;  // 16-B query-row pieces per thread (5 | 4)
  const int mykey = wave * 32;
  bf16x8 qr[QP], orow[QP], kf[4], vf[4];
  // key rows past nk (a short workgroup of the even split): clamped loads, finite, and their dS
  // columns are written as zeros, so they add nothing to dQ.  K^T is staged from the waves' own K
  // fragments (no second read of the K rows)
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    const int c = tid + NT * j;
    const int qq = min(c >> 3, q_count - 1);  // rows past q_count: clamped, never read back
    qr[j] = load8(Q + (size_t)qq * a.q_row + (c & 7) * 8);
    orow[j] = load8(dO + (size_t)qq * a.o_row + (c & 7) * 8);
  }
  const int kfr = min(mykey + r, nk - 1);
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    kf[st] = load8(K + (size_t)kfr * DH + st * 16 + 8 * h);
    vf[st] = load8(V + (size_t)kfr * DH + st * 16 + 8 * h);
  }
  float lsev = 0.f, ddv = 0.f;
  if (tid < LY::MAXQ) {
    const int qq = min(tid, q_count - 1);
    lsev = lse[qq];
    ddv = dd[qq] + (dd2 ? dd2[qq] : 0.f);
  }
  __builtin_amdgcn_sched_barrier(0);
  stamp(1);
#pragma unroll
  for (int st = 0; st < 4; ++st) {   // this lane's key mykey + r, d = 16 st + 8 h .. + 7
#pragma unroll
    for (int e = 0; e < 8; ++e) kt_s[(st * 16 + 8 * h + e) * KT_ROW + mykey + r] = kf[st][e];
  }
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    const int c = tid + NT * j, row = c >> 3, d0 = (c & 7) * 8;
    if (row < LY::MAXQ) {
      *(bf16x8*)(qs + row * QROW + d0) = qr[j];
      *(bf16x8*)(os + row * QROW + d0) = orow[j];
    }
  }
  if (tid < LY::MAXQ) {
    lse_s[tid] = lsev;
    dd_s[tid] = ddv;
  }
  __syncthreads();
  stamp(2);

  f32x16 dvt[2], dkt[2];  // [d tile], cols = this wave's 32 keys
#pragma unroll
  for (int i = 0; i < 2; ++i) { dvt[i] = (f32x16){}; dkt[i] = (f32x16){}; }

#pragma unroll 1
  for (int c0 = 0; c0 < q_count; c0 += 32) {
    // S = Q K^T, dP = dO V^T: rows = queries (registers), cols = this wave's keys (lanes)
    f32x16 s = (f32x16){}, dp = (f32x16){};
    cstamp(c0, 0);
    if (active) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const bf16x8 qa_f = *(const bf16x8*)(qs + (c0 + r) * QROW + st * 16 + 8 * h);
        const bf16x8 oa_f = *(const bf16x8*)(os + (c0 + r) * QROW + st * 16 + 8 * h);
        mma16(s, qa_f, kf[st]);
        mma16(dp, oa_f, vf[st]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int qq = c0 + acc_row(i, h);
        const float p = __expf(s[i] - lse_s[qq]);
        s[i] = p;
        dp[i] = p * (dp[i] - dd_s[qq]);
      }
      // dV^T += dO^T P ; dK^T += Q^T dS
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        const bf16x8 bp = acc_as_operand<bf16>(s, sp);
        const bf16x8 bs = acc_as_operand<bf16>(dp, sp);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16x8 ao = frag_tr_acc(os + c0 * QROW, dt * 32, 16 * sp, lane);
          const bf16x8 aq = frag_tr_acc(qs + c0 * QROW, dt * 32, 16 * sp, lane);
          mma16(dvt[dt], ao, bp);
          mma16(dkt[dt], aq, bs);
        }
      }
    }
    cstamp(c0, 1);
    __syncthreads();  // previous chunk's dQ reads of ds_s are done
    cstamp(c0, 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) ds_s[acc_row(i, h) * DS_ROW + mykey + r] = from_f<bf16>(dp[i]);  // 0: idle wave
    __syncthreads();
    cstamp(c0, 3);
    {
      // waves W0, W0 + 1 (SIMDs that do not host the 9-wave form's ninth wave): d tile wave - W0
      constexpr int W0 = NW == 9 ? 1 : 0;
      if (wave == W0 || wave == W0 + 1) {
        const int dtq = wave - W0;
        f32x16 acc = (f32x16){};
        // software-pipelined: the operand reads of k-steps st + 2, st + 3 are issued before the
        // MFMAs of st, st + 1 (left to itself the compiler sinks each pair of reads to its MFMAs and
        // waits on them: A1 backward 38.5 -> 37.7 us, A3 32.9 -> 32.6, bitwise the same)
        constexpr int NS = 2 * NW;
        const bf16* da = ds_s + r * DS_ROW + 8 * h;
        const bf16* kb = kt_s + (dtq * 32 + r) * KT_ROW + 8 * h;
        bf16x8 fa[4], fb[4];
#pragma unroll
        for (int st = 0; st < 2; ++st) { fa[st] = load8(da + st * 16); fb[st] = load8(kb + st * 16); }
#pragma unroll
        for (int st = 0; st < NS; st += 2) {
#pragma unroll
          for (int u = 2; u < 4; ++u)
            if (st + u < NS) { fa[(st + u) & 3] = load8(da + (st + u) * 16); fb[(st + u) & 3] = load8(kb + (st + u) * 16); }
          __builtin_amdgcn_sched_barrier(0);
          mma16(acc, fa[st & 3], fb[st & 3]);
          if (st + 1 < NS) mma16(acc, fa[(st + 1) & 3], fb[(st + 1) & 3]);
          __builtin_amdgcn_sched_barrier(0);
        }
        cstamp(c0, 4);
        if (MODE == MODE_A1 && a.dqkv) {
          const int bag = bh / nh, hh = bh % nh, ld = 3 * nh * DH;
          bf16* qo = (bf16*)a.dqkv + ((size_t)bag * a.q_total + q_begin + c0) * ld + hh * DH + dtq * 32 + r;
#pragma unroll
          for (int i = 0; i < 16; ++i) qo[(size_t)acc_row(i, h) * ld] = (bf16)(a.dq_scale * acc[i]);
        } else if (MODE == MODE_A3 && a.slab_bf16) {   // the fused A3 backward's dq~ partials as bf16
          bf16* dst = (bf16*)a.dq + (size_t)blk * a.slab_stride + bh * a.dq_bh + (size_t)(q_begin + c0) * DH + dtq * 32 + r;
#pragma unroll
          for (int i = 0; i < 16; ++i) dst[(size_t)acc_row(i, h) * DH] = (bf16)acc[i];
        } else {
          float* dst = MODE == MODE_A1 ? a.dq + bh * a.dq_bh : a.dq + (size_t)blk * a.slab_stride + bh * a.dq_bh;
          dst += (size_t)(q_begin + c0) * DH + dtq * 32 + r;
#pragma unroll
          for (int i = 0; i < 16; ++i) dst[(size_t)acc_row(i, h) * DH] = acc[i];
        }
        cstamp(c0, 5);
      }
    }
    if (c0 == 0) stamp(3);
    if (c0 == 96) stamp(4);
  }
  stamp(5);
  // ---- key-side epilogue through LDS (transpose to [key][d]) ----
  __syncthreads();
  if (MODE == MODE_A3 && a.dqkv) {
    // fused: the final bf16 k / v rows of dqkv (no fp32 key-side slabs, no assemble pass for them):
    // the conv backward's dv window loads issued first, dV and dK staged side by side, the dk~ / l
    // loads, one barrier, then 16-B bf16 stores of 8 columns per item
    constexpr int IT = (LY::NK * DH / 8 + NT - 1) / NT;
    static_assert(2 * LY::NK * 68 * 4 <= LY::BYTES, "fused A3 epilogue: two staged tiles exceed the layout");
    const int bag = bh / nh, hh = bh % nh, inner = nh * DH;
    bf16* outk = (bf16*)a.dqkv + ((size_t)bag * a.n_key_rows + key0) * 3 * inner + inner + hh * DH;
    bf16* outv = outk + inner;
    const bf16* dvc = (const bf16*)a.dv + bh * a.dv_bh + (size_t)key0 * DH;   // the conv backward's dv (bf16)
    const float* dkl = a.dkl + (size_t)bh * NL * DH;
    f32x4 av[IT][2], ak[IT][2];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + NT * it, key = i >> 3, d8 = (i & 7) * 8;
      const bool valid = key < nk;
      const bool vw = valid && key0 + key >= a.dv_lo && key0 + key < a.dv_hi;
      const bf16x8 pv = vw ? *(const bf16x8*)(dvc + (size_t)min(key, nk - 1) * DH + d8) : (bf16x8){};
      av[it][0] = (f32x4){(float)pv[0], (float)pv[1], (float)pv[2], (float)pv[3]};
      av[it][1] = (f32x4){(float)pv[4], (float)pv[5], (float)pv[6], (float)pv[7]};
    }
    float* stage_k = stage + LY::NK * 68;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int o = (mykey + r) * 68 + dt * 32 + 8 * g4 + 4 * h;
        *(f32x4*)(stage + o) = (f32x4){dvt[dt][4 * g4], dvt[dt][4 * g4 + 1], dvt[dt][4 * g4 + 2], dvt[dt][4 * g4 + 3]};
        *(f32x4*)(stage_k + o) = (f32x4){dkt[dt][4 * g4], dkt[dt][4 * g4 + 1], dkt[dt][4 * g4 + 2], dkt[dt][4 * g4 + 3]};
      }
    // dk~ / l rows (L2-resident: 256 x 64 per head) once dV / dK have left the registers
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + NT * it, key = min(i >> 3, nk - 1), d8 = (i & 7) * 8;
      const float* pk = dkl + (size_t)((key0 + key) / a.l) * DH + d8;
      ak[it][0] = *(const f32x4*)pk;
      ak[it][1] = *(const f32x4*)(pk + 4);
    }
    __syncthreads();
    const float il = a.inv_l;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + NT * it, key = i >> 3, d8 = (i & 7) * 8;
      if (key >= nk) continue;
      const float* sv = stage + key * 68 + d8;
      const float* sk = stage_k + key * 68 + d8;
      const f32x4 v0 = *(const f32x4*)sv + av[it][0], v1 = *(const f32x4*)(sv + 4) + av[it][1];
      const f32x4 k0 = *(const f32x4*)sk + ak[it][0] * il, k1 = *(const f32x4*)(sk + 4) + ak[it][1] * il;
      *(bf16x8*)(outv + (size_t)key * 3 * inner + d8) =
          (bf16x8){(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3], (bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
      *(bf16x8*)(outk + (size_t)key * 3 * inner + d8) =
          (bf16x8){(bf16)k0[0], (bf16)k0[1], (bf16)k0[2], (bf16)k0[3], (bf16)k1[0], (bf16)k1[1], (bf16)k1[2], (bf16)k1[3]};
    }
    stamp(6);
    return;
  }
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const f32x16& accv = which == 0 ? dvt[dt] : dkt[dt];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *(f32x4*)(stage + (mykey + r) * 68 + dt * 32 + 8 * g4 + 4 * h) =
            (f32x4){accv[4 * g4], accv[4 * g4 + 1], accv[4 * g4 + 2], accv[4 * g4 + 3]};
    }
    __syncthreads();
    if (MODE == MODE_A1 && a.slab_bf16) {
      bf16* dstb = (bf16*)(which == 0 ? a.dv : a.dk) + (size_t)blk * a.slab_stride + bh * (which == 0 ? a.dv_bh : a.dk_bh);
      for (int i = tid; i < nk * DH / 4; i += NT) {
        const int key = i >> 4, d4 = (i & 15) * 4;
        const f32x4 val = *(const f32x4*)(stage + key * 68 + d4);
        *(bf16x4*)(dstb + (size_t)key * DH + d4) = (bf16x4){(bf16)val[0], (bf16)val[1], (bf16)val[2], (bf16)val[3]};
      }
      __syncthreads();
      continue;
    }
    float* dst;
    bool add = false;
    if (MODE == MODE_A3) {
      dst = (which == 0 ? a.dv + bh * a.dv_bh : a.dk + bh * a.dk_bh) + (size_t)key0 * DH;
      add = (which == 0);
    } else {
      dst = (which == 0 ? a.dv : a.dk) + (size_t)blk * a.slab_stride + bh * (which == 0 ? a.dv_bh : a.dk_bh);
    }
    for (int i = tid; i < nk * DH / 4; i += NT) {
      const int key = i >> 4, d4 = (i & 15) * 4;
      f32x4 val = *(const f32x4*)(stage + key * 68 + d4);
      float* p = dst + (size_t)key * DH + d4;
      if (add) val += *(const f32x4*)p;
      *(f32x4*)p = val;
    }
    __syncthreads();
  }
  stamp(6);
}

}  // namespace
