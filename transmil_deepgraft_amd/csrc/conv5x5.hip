// The two convolution stages of the `simple` tile backbone (the MIL-AB embedder of
// code/models/model_interface.py:270-281) in one pass each:
//
//   out = maxpool2x2/2(relu(conv5x5_valid(x, w) + bias))        (3 -> 20 and 20 -> 50 channels)
//
// stride 1, no padding, floor-mode pool (an odd convolution output drops its last row / column).
// The convolution output never reaches HBM.
//
// Both stages are one templated implicit GEMM on the MFMA units, the output channels on the MFMA
// rows (A = the packed weights, NU tiles of 32 rows: 20 -> 32, 50 -> 64) and 32 convolution pixels
// of one row on its columns (B).  A workgroup (256 threads) owns a 4 RT x 32 patch of convolution
// pixels = 2 RT x 16 pooled pixels of one tile (RT = 4; 2 in the f32 second stage, whose accumulators
// are twice as many); wave v owns convolution rows RT v .. RT v + RT - 1 of it, so the vertical max
// of a pool window is a register-wise max of two of the wave's accumulator tiles and the horizontal
// max one DPP lane swap (columns l, l ^ 1): no LDS round trip for the pool.  A weight fragment is
// loaded once per k-step and feeds RT MFMAs.  Bias and ReLU come after the max (x -> fl(x + b) and
// the ReLU are monotone, so they commute with it bitwise), then one rounding and the store.
//
// LDS image: the (4 RT + 4)-row input window of the patch, channels-last, [4 RT + 4][WINW] pixels of
// CPIX elements:
//   3 -> 20:  CPIX = 4 (the three channels + a zero), WINW = 37, read from any (n, c, h, w) element
//             strides.  A k fragment (8 consecutive k of one lane half) = 2 adjacent pixels x 4
//             channels: 3 fragments per kernel row (kx = 0..5, kx = 5 and channel 3 carry zero
//             weights), 15 fragments, K padded to 16 fragments = 8 MFMA k-steps.
//   20 -> 50: CPIX = 24 (the first stage's output layout: 20 channels + 4 written as zeros), WINW = 36,
//             staged as 16-B pieces.  A fragment = 8 channels of one tap's pixel: 3 fragments per tap,
//             75 fragments, K padded to 76 = 38 k-steps (K = 608 for the 500 that carry weight).
// Lane (column l, half h) reads fragment 2s + h of k-step s at the constant offset of that fragment
// from its own pixel, so the two halves of a wave may read different taps.  bf16 pixels of 48 B put
// 16 consecutive lanes' 16-B reads on distinct banks; the 8-B pixels of the first stage are
// contiguous.  The fragment past the last (zero weights) re-reads fragment 0 (finite data).
// Every window element is a loaded value or zero, so a zero weight never meets LDS garbage.
//
// The weights are packed on the host, once, in fragment order [k-step][row tile][lane][8]: a wave's
// A fragment is one contiguous 1 KB (bf16) read.  The first stage's 8 KB (bf16) / 16 KB are copied to
// LDS once per workgroup; the second stage's 78 / 156 KB are read by each wave from L1 / L2 into a
// register ring four k-steps (f32: two) ahead of their MFMAs.  The pixel fragments run one k-step
// ahead, and a scheduling barrier per k-step keeps both prefetches where they are written (left to
// itself the compiler kept one weight load in flight: an L2 round trip per k-step).
// The bias sits in LDS (zero past cout) so that the epilogue reads it without a branch.
//
// f32 (the parity mode): v_mfma_f32_32x32x2_f32 with two independent accumulation chains per tile
// (even / odd k element), summed once at the end.  No atomics, fixed order: bitwise reproducible.
// x and out are addressed with 64-bit offsets.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int PC = 16;                    // pooled columns per workgroup
constexpr int kMaxExtent = 1 << 15;

// RT = convolution rows (32-pixel MFMA column tiles) per wave: a weight fragment is loaded once per
// k-step and used by RT MFMAs per row tile
template <int CIN, int RT>
struct Geo {
  static constexpr bool FIRST = CIN == 3;
  static constexpr int PR = 2 * RT;                    // pooled rows per workgroup (RT / 2 per wave)
  static constexpr int WINH = 4 * RT + 4;              // input rows of the window
  static constexpr int CPIX = FIRST ? 4 : 24;          // LDS elements per pixel
  static constexpr int NU = FIRST ? 1 : 2;             // MFMA row tiles (32 output channels each)
  static constexpr int NG = FIRST ? 5 : 25;            // groups of 3 fragments (kernel rows / taps)
  static constexpr int NF = 3 * NG;                    // fragments that carry weight
  static constexpr int NS = (NF + 1) / 2;              // k-steps of 16
  static constexpr int WINW = FIRST ? 2 * PC + 5 : 2 * PC + 4;
  static constexpr int NPIX = WINH * WINW;
  static constexpr int WELEMS = NS * NU * 64 * 8;      // packed weight elements
  // element offset of fragment f from the lane's own pixel
  static __host__ __device__ constexpr int foff(int f) {
    if (f >= NF) return 0;
    const int g = f / 3, sub = f % 3;
    return (FIRST ? g * WINW * 4 : ((g / 5) * WINW + g % 5) * 24) + sub * 8;
  }
};

struct Conv5x5Params {
  const void* x; const void* wp; const float* bias; void* out;
  long long sn, sc, sh, sw, so;
  int h, w, ph, pw, nbr, nbc, cout, cpo, tail;
};

typedef float f32x2v __attribute__((ext_vector_type(2)));

template <typename T> TM_DEV void store2(T* p, float a, float b);
template <> TM_DEV void store2<float>(float* p, float a, float b) { *(f32x2v*)p = (f32x2v){a, b}; }
template <> TM_DEV void store2<bf16>(bf16* p, float a, float b) { *(bf16x2*)p = (bf16x2){(bf16)a, (bf16)b}; }

// 8 consecutive LDS elements at an 8-byte (bf16, first stage) or 16-byte aligned address
template <typename T, bool AL16>
TM_DEV vec8<T> ldfrag(const T* p) {
  if constexpr (AL16 || sizeof(T) == 4) {
    return load8<T>(p);
  } else {
    const vec4<T> a = load4<T>(p), b = load4<T>(p + 4);
    return (vec8<T>){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  }
}

// one element's bits, zero-extended into a register of its own
TM_DEV unsigned ldraw(const bf16* p) { return *(const unsigned short*)p; }
TM_DEV unsigned ldraw(const float* p) { return __builtin_bit_cast(unsigned, *p); }
// an LDS pixel of the first stage: the three channel values + a zero
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
TM_DEV void stpix(bf16* d, unsigned a, unsigned b, unsigned c) { *(u32x2*)d = (u32x2){a | (b << 16), c}; }
TM_DEV void stpix(float* d, unsigned a, unsigned b, unsigned c) { *(u32x4*)d = (u32x4){a, b, c, 0u}; }

template <typename T, int CIN, int RT>
__global__ __launch_bounds__(kThreads) void conv5x5_kernel(const Conv5x5Params p) {
  using G = Geo<CIN, RT>;
  constexpr int PR = G::PR;
  constexpr int E = 16 / (int)sizeof(T);          // elements per 16-B piece
  constexpr int NP = sizeof(T) == 4 ? 2 : 1;      // accumulation chains per tile
  // the first stage's 8 / 16 KB of weights go through LDS once per workgroup; the second stage's
  // 78 / 156 KB are read by each wave from L1 / L2 (the register ring below)
  constexpr bool WLDS = G::FIRST;
  __shared__ __attribute__((aligned(16))) T win[G::NPIX * G::CPIX];
  __shared__ __attribute__((aligned(16))) T wl[WLDS ? G::WELEMS : 8];
  __shared__ float bl[32 * G::NU];                // the bias, zero past cout

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const unsigned bid = blockIdx.x;
  const int ppt = p.nbr * p.nbc;
  const long long n = bid / ppt;
  const int rem = (int)(bid - n * ppt);
  const int br = rem / p.nbc, bc = rem - br * p.nbc;
  const int pr0 = br * PR, pc0 = bc * PC;
  const int iy0 = 2 * pr0, ix0 = 2 * pc0;         // the window's first input row / column

  const T* __restrict__ x = (const T*)p.x + n * p.sn;
  T* __restrict__ out = (T*)p.out + n * p.so;

  // (loaded before the window so that it shares the window's memory round trip)
  const float bv = tid < p.cout ? p.bias[min(tid, p.cout - 1)] : 0.f;
  if constexpr (WLDS) {
    constexpr int NW = (G::WELEMS / E + kThreads - 1) / kThreads;
    f32x4 wr[NW];
#pragma unroll
    for (int t = 0; t < NW; ++t) wr[t] = *(const f32x4*)((const T*)p.wp + min(tid + t * kThreads, G::WELEMS / E - 1) * E);
#pragma unroll
    for (int t = 0; t < NW; ++t)
      if (tid + t * kThreads < G::WELEMS / E) *(f32x4*)(wl + (tid + t * kThreads) * E) = wr[t];
  }
  // ---- the input window -> LDS (zero outside the tile).  Every load of a thread is issued before
  // its first LDS store (one memory round trip, not one per piece), unconditionally: the coordinates
  // of a piece outside the tile are clamped into it and its value is replaced by zero
  if constexpr (G::FIRST) {
    // (each channel value in a 32-bit register of its own: a 16-bit load into half a register
    // would wait for the load of the other half)
    constexpr int NT = (G::NPIX + kThreads - 1) / kThreads;
    unsigned r[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = min(tid + t * kThreads, G::NPIX - 1);
      const int gy = iy0 + i / G::WINW, gx = ix0 + i % G::WINW;
      const unsigned keep = gy < p.h && gx < p.w ? 0xFFFFFFFFu : 0u;
      const T* q = x + min(gy, p.h - 1) * p.sh + min(gx, p.w - 1) * p.sw;
#pragma unroll
      for (int c = 0; c < 3; ++c) r[t][c] = ldraw(q + c * p.sc) & keep;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = tid + t * kThreads;
      if (i < G::NPIX) stpix(win + i * 4, r[t][0], r[t][1], r[t][2]);
    }
  } else {
    constexpr int PP = G::CPIX / E;               // 16-B pieces per pixel
    constexpr int NT = (G::NPIX * PP + kThreads - 1) / kThreads;
    f32x4 r[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = min(tid + t * kThreads, G::NPIX * PP - 1);
      const int pix = i / PP, piece = i - pix * PP;
      const int gy = iy0 + pix / G::WINW, gx = ix0 + pix % G::WINW;
      const bool ok = gy < p.h && gx < p.w;
      const f32x4 v = *(const f32x4*)(x + min(gy, p.h - 1) * p.sh + min(gx, p.w - 1) * p.sw + piece * E);
      r[t] = ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = tid + t * kThreads;
      if (i < G::NPIX * PP) *(f32x4*)(win + i * E) = r[t];
    }
  }
  if (tid < 32 * G::NU) bl[tid] = bv;
  // the zero tail of the tile's output row (the K padding of the Linear's A matrix)
  if (rem == 0) {
    T* tl = out + (long long)p.ph * p.pw * p.cpo;
    for (int i = tid; i < p.tail; i += kThreads) tl[i] = from_f<T>(0.f);
  }
  __syncthreads();

  // ---- k loop: wave = convolution rows RT wave + t (t = 0 .. RT - 1), lane = column l32
  f32x16 acc[RT][G::NU][NP];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int u = 0; u < G::NU; ++u)
#pragma unroll
      for (int q = 0; q < NP; ++q) acc[t][u][q] = (f32x16){};

  const T* __restrict__ wp = (WLDS ? (const T*)wl : (const T*)p.wp) + lane * 8;
  const T* b0 = win + ((RT * wave) * G::WINW + l32) * G::CPIX;
  // weights read from memory run WD k-steps ahead of their MFMAs in a register ring (an L2 round
  // trip is several k-steps long)
  constexpr int WD = WLDS ? 1 : (sizeof(T) == 4 ? 2 : 4);
  vec8<T> wq[WD][G::NU];
  if constexpr (!WLDS) {
#pragma unroll
    for (int s = 0; s < WD; ++s)
#pragma unroll
      for (int u = 0; u < G::NU; ++u) wq[s][u] = load8<T>(wp + (s * G::NU + u) * 64 * 8);
  }
  // the pixel fragments run one k-step ahead (two register sets); a scheduling barrier per k-step
  // keeps the compiler from sinking either prefetch back to its use
  vec8<T> xf[2][RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) xf[0][t] = ldfrag<T, !G::FIRST>(b0 + t * G::WINW * G::CPIX + (hh ? G::foff(1) : G::foff(0)));
#pragma unroll
  for (int s = 0; s < G::NS; ++s) {
    if (s + 1 < G::NS) {
      const int o = hh ? G::foff(2 * s + 3) : G::foff(2 * s + 2);
#pragma unroll
      for (int t = 0; t < RT; ++t) xf[(s + 1) & 1][t] = ldfrag<T, !G::FIRST>(b0 + t * G::WINW * G::CPIX + o);
    }
#pragma unroll
    for (int u = 0; u < G::NU; ++u) {
      vec8<T> wf;
      if constexpr (WLDS) wf = load8<T>(wp + (s * G::NU + u) * 64 * 8);
      else wf = wq[s % WD][u];
      if constexpr (NP == 1) {
#pragma unroll
        for (int t = 0; t < RT; ++t) mma16(acc[t][u][0], wf, xf[s & 1][t]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[t][u][j & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j], xf[s & 1][t][j], acc[t][u][j & 1], 0, 0, 0);
      }
      if constexpr (!WLDS) {
        if (s + WD < G::NS) wq[s % WD][u] = load8<T>(wp + ((s + WD) * G::NU + u) * 64 * 8);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- pool, bias, ReLU, store: even lanes own pooled pixels (pr0 + wave RT / 2 + v, pc0 + l32 / 2),
  // v = 0 .. RT / 2 - 1 (row tiles 2 v and 2 v + 1); register 4 k + e of row tile u is channel
  // 32 u + 8 k + 4 hh + e
  const int pc = pc0 + (l32 >> 1);
#pragma unroll
  for (int v = 0; v < RT / 2; ++v) {
  const int pr = pr0 + wave * (RT / 2) + v;
  const bool own = (l32 & 1) == 0 && pr < p.ph && pc < p.pw;
  T* o = out + ((long long)pr * p.pw + pc) * p.cpo;
#pragma unroll
  for (int u = 0; u < G::NU; ++u) {
    f32x16 m;
    if constexpr (NP == 2) {
      const f32x16 r0 = acc[2 * v][u][0] + acc[2 * v][u][1], r1 = acc[2 * v + 1][u][0] + acc[2 * v + 1][u][1];
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = fmaxf(r0[i], r1[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = fmaxf(acc[2 * v][u][0][i], acc[2 * v + 1][u][0][i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = fmaxf(m[i], dpp_mov<0xB1>(0.f, m[i]));   // quad_perm [1, 0, 3, 2]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 32 * u + 8 * k + 4 * hh;
      if (!own || c >= p.cpo) continue;
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = fmaxf(m[4 * k + e] + bl[c + e], 0.f);
      store2<T>(o + c, r[0], r[1]);
      if (c + 2 < p.cpo) store2<T>(o + c + 2, r[2], r[3]);
    }
  }
  }
}

// 4 convolution rows per wave except the f32 second stage (2: its 2 x 2 accumulator tiles per row
// already take 128 registers)
template <typename T, int CIN>
constexpr int rows_per_wave() { return sizeof(T) == 4 && CIN == 20 ? 2 : 4; }

template <typename T, int CIN>
int launch(Conv5x5Params& p, long long n, hipStream_t st) {
  constexpr int RT = rows_per_wave<T, CIN>();
  using G = Geo<CIN, RT>;
  p.nbr = (p.ph + G::PR - 1) / G::PR; p.nbc = (p.pw + PC - 1) / PC;
  const long long blocks = n * p.nbr * p.nbc;
  TM_REQUIRE(blocks < (1LL << 31), "conv5x5: too many output patches for one launch (n * h * w too large)");
  hipLaunchKernelGGL((conv5x5_kernel<T, CIN, RT>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p);
  TM_CHECK_LAUNCH();
  return 0;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int tm_conv5x5_relu_pool(int dtype, const void* x, const void* wp, const float* bias, void* out,
                                    long long n, int h, int w, int cin, int cout, long long sn, long long sc,
                                    long long sh, long long sw, long long so, int cpo, int tail, void* stream) {
  TM_REQUIRE(dtype == TM_BF16 || dtype == TM_F32, "conv5x5: dtype must be TM_F32 or TM_BF16");
  TM_REQUIRE((cin == 3 && cout == 20) || (cin == 20 && cout == 50), "conv5x5: (cin, cout) must be (3, 20) or (20, 50)");
  TM_REQUIRE(h >= 6 && w >= 6 && h <= kMaxExtent && w <= kMaxExtent, "conv5x5: h and w must be in 6..32768");
  TM_REQUIRE(n >= 1 && n < (1LL << 40), "conv5x5: n must be in 1..2^40");
  TM_REQUIRE(x && wp && bias && out, "conv5x5: x, wp, bias and out must not be NULL");
  const int esz = dtype == TM_BF16 ? 2 : 4;
  TM_REQUIRE(aligned16(wp) && aligned16(out) && ((uintptr_t)bias & 3) == 0 && ((uintptr_t)x % esz) == 0,
             "conv5x5: wp and out must be 16-byte aligned (x and bias element aligned)");
  TM_REQUIRE(sn > 0 && sc > 0 && sh > 0 && sw > 0, "conv5x5: input strides must be positive");
  const int ph = (h - 4) / 2, pw = (w - 4) / 2;
  TM_REQUIRE(cpo % 2 == 0 && cpo >= cout && cpo <= (cin == 3 ? 32 : 64),
             "conv5x5: cpo must be even, >= cout and <= 32 (3 -> 20) / 64 (20 -> 50)");
  TM_REQUIRE(tail >= 0 && so % 2 == 0 && so >= (long long)ph * pw * cpo + tail,
             "conv5x5: the output tile stride must be even and hold ph * pw * cpo + tail elements");
  if (cin == 20)
    TM_REQUIRE(sc == 1 && sw == 24 && sh % 8 == 0 && sn % 8 == 0 && sh >= 24LL * w && aligned16(x),
               "conv5x5: the 20 -> 50 stage reads 16-byte aligned channels-last pixels of 24 channels (sc = 1, sw = 24, "
               "sh and sn multiples of 8)");
  Conv5x5Params p;
  p.x = x; p.wp = wp; p.bias = bias; p.out = out;
  p.sn = sn; p.sc = sc; p.sh = sh; p.sw = sw; p.so = so;
  p.h = h; p.w = w; p.ph = ph; p.pw = pw;
  p.nbr = 0; p.nbc = 0;
  p.cout = cout; p.cpo = cpo; p.tail = tail;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) return cin == 3 ? launch<bf16, 3>(p, n, st) : launch<bf16, 20>(p, n, st);
  return cin == 3 ? launch<float, 3>(p, n, st) : launch<float, 20>(p, n, st);
}
