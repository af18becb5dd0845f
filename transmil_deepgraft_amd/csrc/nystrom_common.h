// What the two compute modes of the NystromAttention core share (included by nystrom.hip, the one
// translation unit, ahead of nystrom_f32.h and nystrom_bf16.h): the fixed geometry, the LDS
// layouts of keys and values (Lay), the value fragment loaders of the P.V product (value_frag),
// the register-held [256][64] tile (TileRegs), the softmax row trees (tree_max16 / tree_sum16)
// and the argument block of the shared flash-style backward (BwdArgs, MODE_A1 / MODE_A3).
#pragma once
#include "common.h"

namespace {

constexpr int DH = 64;     // dim_head
constexpr int NL = 256;    // landmarks
constexpr int TAPS = 33;   // residual conv kernel
constexpr int HALF = 16;   // conv padding

// LDS row strides (elements).  Keys [256][KROW]: 144 B (bf16) / 272 B (f32) rows
// -> conflict-free ds_read_b128 for 16 consecutive rows.
// Values, bf16: natural [256 keys][VROW = 80] (160-B rows: the transposing
// ds_read_b64_tr_b16 of 4 keys x 16 d hits 64 distinct banks per 32-lane half);
// fp32 (parity mode, no 32-bit transposing read): values^T [64][VROW = 260].
template <typename T> struct Lay {
  static constexpr int KROW = DH + 16 / (int)sizeof(T);    // 72 bf16 / 68 f32
  static constexpr int VROW = sizeof(T) == 2 ? 80 : NL + 4;
  static constexpr int VELEMS = sizeof(T) == 2 ? NL * VROW : DH * VROW;
};

TM_DEV long long hoff(long long bh, int nh, long long bag_stride, long long head_stride) {
  return (bh / nh) * bag_stride + (bh % nh) * head_stride;
}

// A operand of O^T = V^T P^T for d tile dt and the 16-key step starting at key kb:
// element j of lane (r, h) = V[kb + 8(j>>2) + 4h + (j&3)][dt*32 + r]  (acc_k_index order).
template <typename T> TM_DEV vec8<T> value_frag(const T* vs, int dt, int kb, int lane);
template <> TM_DEV bf16x8 value_frag<bf16>(const bf16* vs, int dt, int kb, int lane) {
  // natural [key][80] layout, two transposing reads of 4 keys x 16 d
  constexpr int VROW = Lay<bf16>::VROW;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int d = dt * 32 + (g & 1) * 16 + 4 * p;
  const int key = kb + 4 * (g >> 1) + q;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(vs + key * VROW + d));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(vs + (key + 8) * VROW + d));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <> TM_DEV f32x8 value_frag<float>(const float* vt, int dt, int kb, int lane) {
  // transposed [d][260] layout
  constexpr int VROW = Lay<float>::VROW;
  const float* row = vt + (dt * 32 + (lane & 31)) * VROW + kb + 4 * (lane >> 5);
  const f32x4 lo = *(const f32x4*)row, hi = *(const f32x4*)(row + 8);
  return (f32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// softmax rows of a score tile: exp as exp2 of one fma (LOG2E), max and sum as balanced trees
constexpr float LOG2E = 1.4426950408889634f;

// 16-element max as v_max3_f32 triples (8 instructions instead of 15)
TM_DEV float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
TM_DEV float tree_max16(const f32x16& x) {
  const float m0 = max3f(x[0], x[1], x[2]), m1 = max3f(x[3], x[4], x[5]), m2 = max3f(x[6], x[7], x[8]);
  const float m3 = max3f(x[9], x[10], x[11]), m4 = max3f(x[12], x[13], x[14]);
  return __builtin_fmaxf(max3f(m0, m1, m2), max3f(m3, m4, x[15]));
}
// 16-element sum with packed adds (v_pk_add_f32: two lanes of the tree per instruction)
TM_DEV float tree_sum16(const f32x16& x) {
  f32x2 a[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    a[i] = (f32x2){x[2 * i], x[2 * i + 1]} + (f32x2){x[2 * i + 8], x[2 * i + 9]};
  a[0] += a[2];
  a[1] += a[3];
  a[0] += a[1];
  return a[0][0] + a[0][1];
}

// A [256][64] T tile (row stride 64) held in registers between its global loads and its
// LDS writes: a compile-time count of 16-B pieces per thread, so every load of the tile is
// issued before the first wait (a runtime-bounded `for (i = tid; ...)` loop let the compiler
// pipeline only the first few and serialise the rest, one HBM/L2 round trip each).  Both modes
// stage through it: the fp32 kernels as TileRegs<float>, a1_fwd_bf16_kernel as TileRegs<bf16>.
template <typename T, int NT = 256>
struct TileRegs {
  static constexpr int E = 16 / sizeof(T), PER_ROW = DH / E, PER = NL * PER_ROW / NT;
  f32x4 r[PER];
  TM_DEV void load(const T* src, int tid) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + NT * j;
      r[j] = *(const f32x4*)(src + (size_t)(i / PER_ROW) * DH + (i % PER_ROW) * E);
    }
  }
  // keys: ks[key][KROW]
  TM_DEV void store_keys(T* ks, int tid) const {
    constexpr int KROW = Lay<T>::KROW;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + NT * j;
      *(f32x4*)(ks + (i / PER_ROW) * KROW + (i % PER_ROW) * E) = r[j];
    }
  }
  // values in the layout of Lay<T> (bf16 natural [key][VROW], fp32 transposed [d][VROW])
  TM_DEV void store_values(T* vs, int tid) const {
    constexpr int VROW = Lay<T>::VROW;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + NT * j, key = i / PER_ROW, d0 = (i % PER_ROW) * E;
      if constexpr (sizeof(T) == 2) {
        *(f32x4*)(vs + key * VROW + d0) = r[j];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) vs[(d0 + e) * VROW + key] = r[j][e];
      }
    }
  }
};

// ---------------------------------------------------------------------------
// Flash-style backward shared by both attention products.  A workgroup owns a
// block of 256 keys (4 waves x 64, key on the MFMA lane) and walks query chunks
// of 32.  With P = exp(Q K^T - lse), dS = P (dO V^T - D):
//   dV^T += dO^T P,  dK^T += Q^T dS   (registers, sum over the walked queries)
//   dQ    = dS K                      (per chunk, dS through LDS)
// MODE_A3: keys = k rows (block kb), queries = all 256 landmarks;
//          dK -> dk (=), dV -> dv (+=), dQ -> partial slab [kb] (dql).
// MODE_A1: keys = the 256 landmarks, queries = rows [qc*QC, (qc+1)*QC);
//          dQ -> dq (=), dK -> partial slab [qc] (dkl), dV -> partial slab [qc] (dY).
struct BwdArgs {
  const void* q; long long q_bag, q_head; int q_row;    // queries (T)
  const void* dO; long long o_bag, o_head; int o_row;   // upstream grad (T)
  const void* k; long long k_bag, k_head;               // keys (T), row stride 64
  const void* v; long long v_bag, v_head;               // values (T), row stride 64
  const float* lse;  long long lse_bh;                  // [bh][...]
  const float* dd;   long long dd_bh;                   // D per query
  const float* dd2;                                     // optional second partial of D (summed: dd + dd2)
  float* dq; long long dq_bh;                           // query-side grad (fp32, row stride 64)
  float* dk; long long dk_bh;                           // key-side grads (fp32, row stride 64)
  float* dv; long long dv_bh;
  long long slab_stride;                                // per block partial slab stride (MODE dependent)
  int nh, n_queries_per_wg, n_key_rows;
  int q_total;  // bf16 A1 kernel: > 0 = split the q_total / 32 query chunks evenly over gridDim.x
  // bf16 A3 kernel, fused key side: non-null = write the FINAL k / v parts of dqkv (bf16,
  // [bag][n][3 nh 64]): k = dK + dk~[t / l] / l, v = dv (the conv backward's, read) + dV
  void* dqkv; const float* dkl; float inv_l; int l;
  int dv_lo, dv_hi;   // fused: rows of the conv backward's dv that are read (zero outside)
  // bf16 A1 kernel: dqkv non-null = dq written as bf16(dq_scale * dq) into the q part of dqkv
  // ([bag][q_total][3 nh 64], the columns of head bh % nh) instead of fp32 rows at dq
  float dq_scale;
  // 1 = partial slabs written as bf16 (half the slab bytes out and back; their consumers sum them in
  // fp32): the bf16 A1 kernel's dk~ / dY slabs (through the deferred flush), the fused A3 backward's
  // dq~ slab (through assemble_q_slab / cls_q_rows); the slab strides then count bf16 elements
  int slab_bf16;
};

enum { MODE_A3 = 0, MODE_A1 = 1 };
}  // namespace
