// 3x3 convolution (pad 1, stride 1 or 2) over channels-last activations as an implicit GEMM on
// the MFMA units: the ResNet-18 tile encoder's BasicBlock convolutions (16 of its 20, 92 % of its
// FLOPs), BatchNorm folded into w / bias, with the block's residual and ReLU in the epilogue.
//
//   y[n, oy, ox, co] = act(sum_{ky,kx,ci} x[n, oy*s + ky - 1, ox*s + kx - 1, ci] * w[co][ky][kx][ci]
//                          + bias[co] + residual[n, oy, ox, co])
//
// GEMM view: M = n*ho*wo output pixels, N = cout, K = 9*cin.  One workgroup (256 threads, 2 x 2
// waves) owns 128 output pixels x 64 output channels; the pixels are a TH x TW patch (TW = 8 / 16 /
// 32 / 64 columns picked per layer so that ceil(wo / TW) * TW wastes least, TH = 128 / TW rows of
// the flattened [n*ho] output-row axis: a patch may span tiles, every row is staged on its own).
// K runs over (ky, 128-byte channel slice): per step the workgroup stages
//   * the input ROW WINDOW of each of its TH output rows for this ky: (TW - 1)*s + 3 input pixels
//     x 128 B of channels, zero where the row / column is padding or past the tensor, and
//   * the three kx taps of the weights: 3 x 64 output channels x 128 B,
// once, and the three horizontal taps read their pixel fragments from that one window at shifted
// rows (stride 2: the window is stored even columns first, then odd, so a tap's 32 pixels are
// consecutive LDS rows).  x is read from memory three times (once per ky), not nine.
// LDS rows are gemm.hip's k-contiguous image: 128 B of k + 16 B pad (144 B: ds_read_b128 fragments
// of 32 consecutive rows hit distinct banks); one LDS buffer, the next step's global loads held in
// registers across the MFMAs, two barriers per step (gemm.hip's register-staged loop).
// The weights are the MFMA's A operand and the pixels its B operand, so a lane's accumulator
// registers 4g..4g+3 are four CONSECUTIVE output channels of one pixel: the epilogue adds bias and
// residual, applies the ReLU, rounds once and writes each with one 8-B (bf16) / 16-B (f32) vector
// store -- the block output is written once.  No atomics, fixed summation order: bitwise
// reproducible.  x and y are addressed with 64-bit offsets (a 4096-tile bag at 56 x 56 x 64 is
// 822 M elements).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int BM = 128;          // output pixels per workgroup
constexpr int BN = 64;           // output channels per workgroup
constexpr int ROWB = 128 + 16;   // LDS row: one 128-B k slice + pad
constexpr int kMaxExtent = 1 << 15;

typedef f32x4 raw16;             // 16 bytes in flight between global memory and LDS

template <int TW, int S>
struct Geo {
  static constexpr int TH = BM / TW;
  static constexpr int WIN = (TW - 1) * S + 3;     // input pixels of one row window
  static constexpr int A_ROWS = TH * WIN;
  static constexpr int NA = (A_ROWS * 8 + kThreads - 1) / kThreads;   // 16-B pieces per thread
  static constexpr int B_ROWS = 3 * BN;
  static constexpr int NB = B_ROWS * 8 / kThreads;
  static constexpr int A_BYTES = A_ROWS * ROWB;
  static constexpr int SMEM = (A_ROWS + B_ROWS) * ROWB;
  // LDS row (within one output row's window) of window column j
  static __host__ __device__ constexpr int slot(int j) { return S == 1 ? j : (j & 1) * (TW + 1) + (j >> 1); }
  // ... and of the input pixel tap kx of output column tw reads: slot(tw * S + kx)
  static __device__ __forceinline__ int tap(int tw, int kx) {
    return S == 1 ? tw + kx : (kx == 1 ? TW + 1 + tw : tw + (kx >> 1));
  }
};

struct Conv3x3Params {
  const void* x; const void* w; const void* bias; const void* res; void* y;
  long long rows;                 // n * ho flattened output rows
  int h, wd, ho, wo, cin, cout, relu, nseg, nct;
};

template <typename T, int TW, int S>
__global__ __launch_bounds__(kThreads) void conv3x3_kernel(const Conv3x3Params p) {
  using G = Geo<TW, S>;
  constexpr int E = 16 / (int)sizeof(T);       // elements per 16-B piece
  constexpr int KC = 8 * E;                    // channels per k slice (64 bf16 / 32 f32)
  constexpr int NS = KC / 16;                  // 16-deep MFMA steps per slice
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, hh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;

  const unsigned bid = blockIdx.x;
  const int ct = bid % p.nct;
  const unsigned t = bid / p.nct;
  const int seg = t % p.nseg;
  const long long r0 = (long long)(t / p.nseg) * G::TH;
  const int ox0 = seg * TW, co0 = ct * BN;
  const long long n0 = r0 / p.ho;
  const int oy0 = (int)(r0 - n0 * p.ho);

  const T* __restrict__ x = (const T*)p.x;
  const T* __restrict__ w = (const T*)p.w;

  // ---- what this thread stages each step: NA pieces of the row windows, NB of the weights
  long long aoff[G::NA];   // element offset of the piece at ky = 0, c0 = 0
  int aiy[G::NA];          // its input row at ky = 0 (far negative: never valid)
  int adst[G::NA];
#pragma unroll
  for (int i = 0; i < G::NA; ++i) {
    const int e = tid + i * kThreads;
    const int arow = e >> 3, v = e & 7;
    const int th = arow / G::WIN, j = arow - th * G::WIN;
    const int q = (oy0 + th) / p.ho;
    const int oy = oy0 + th - q * p.ho;
    const long long ni = n0 + q;
    const int ix = ox0 * S - 1 + j;
    const int iy = oy * S - 1;
    const bool ok = arow < G::A_ROWS && r0 + th < p.rows && ix >= 0 && ix < p.wd;
    aoff[i] = ((ni * p.h + iy) * p.wd + ix) * p.cin + v * E;
    aiy[i] = ok ? iy : -(1 << 30);
    adst[i] = arow < G::A_ROWS ? (th * G::WIN + G::slot(j)) * ROWB + v * 16 : -1;
  }
  int boff[G::NB];
#pragma unroll
  for (int i = 0; i < G::NB; ++i) {
    const int e = tid + i * kThreads;
    const int brow = e >> 3, v = e & 7;          // brow = kx * 64 + co
    boff[i] = ((co0 + (brow & 63)) * 9 + (brow >> 6)) * p.cin + v * E;
  }

  raw16 ra[G::NA], rb[G::NB];
  const int nc = p.cin / KC, nit = 3 * nc;
  auto fetch = [&](int it) {
    const int ky = it / nc, c0 = (it - ky * nc) * KC;
    const long long ashift = (long long)ky * p.wd * p.cin + c0;
#pragma unroll
    for (int i = 0; i < G::NA; ++i) {
      const bool ok = (unsigned)(aiy[i] + ky) < (unsigned)p.h;
      ra[i] = ok ? *(const raw16*)(x + aoff[i] + ashift) : (raw16){0.f, 0.f, 0.f, 0.f};
    }
    const int bshift = ky * 3 * p.cin + c0;
#pragma unroll
    for (int i = 0; i < G::NB; ++i) rb[i] = *(const raw16*)(w + boff[i] + bshift);
  };

  // ---- fragment addresses: pixel lr of each of the wave's two 32-pixel groups, channel lr
  int abase[2];
  int atw[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int m = wm * 64 + a * 32 + lr;
    abase[a] = (m / TW) * G::WIN * ROWB + hh * 8 * (int)sizeof(T);
    atw[a] = m % TW;
  }
  const int wbase = G::A_BYTES + (wn * 32 + lr) * ROWB + hh * 8 * (int)sizeof(T);

  // bf16: one fp32 accumulator per 32-pixel group.  f32 (the parity mode): NP = 4 independent
  // chains per group (k-step parity x element parity), summed pairwise at the end -- each chain is
  // a quarter as long, which halves the rounding error of one serial chain over K = 9 cin
  constexpr int NP = sizeof(T) == 4 ? 4 : 1;
  f32x16 acc[2][NP];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][q][i] = 0.f;

  fetch(0);
  for (int it = 0; it < nit; ++it) {
#pragma unroll
    for (int i = 0; i < G::NA; ++i)
      if (adst[i] >= 0) *(raw16*)(smem + adst[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < G::NB; ++i)
      *(raw16*)(smem + G::A_BYTES + ((tid + i * kThreads) >> 3) * ROWB + (tid & 7) * 16) = rb[i];
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int a0 = abase[0] + G::tap(atw[0], kx) * ROWB;
      const int a1 = abase[1] + G::tap(atw[1], kx) * ROWB;
      const int wb = wbase + kx * BN * ROWB;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int ko = s * 16 * (int)sizeof(T);
        const vec8<T> wf = load8<T>((const T*)(smem + wb + ko));
        const vec8<T> x0 = load8<T>((const T*)(smem + a0 + ko));
        const vec8<T> x1 = load8<T>((const T*)(smem + a1 + ko));
        if constexpr (NP == 1) {
          mma16(acc[0][0], wf, x0);
          mma16(acc[1][0], wf, x1);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int q = (s & 1) * 2 + (j & 1);
            acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j], x0[j], acc[0][q], 0, 0, 0);
            acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j], x1[j], acc[1][q], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: registers 4g..4g+3 = channels co .. co+3 of pixel (a, lr)
  const T* __restrict__ bias = (const T*)p.bias;
  const T* __restrict__ res = (const T*)p.res;
  T* __restrict__ y = (T*)p.y;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int m = wm * 64 + a * 32 + lr;
    const int th = m / TW, ox = ox0 + m % TW;
    const long long r = r0 + th;
    if (r >= p.rows || ox >= p.wo) continue;
    const long long pix = (r * p.wo + ox) * p.cout;
    if constexpr (NP == 4) acc[a][0] = (acc[a][0] + acc[a][1]) + (acc[a][2] + acc[a][3]);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = co0 + wn * 32 + 8 * g + 4 * hh;
      float v[4] = {acc[a][0][4 * g], acc[a][0][4 * g + 1], acc[a][0][4 * g + 2], acc[a][0][4 * g + 3]};
      if (bias) {
        const vec4<T> b = load4<T>(bias + co);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += to_f(b[k]);
      }
      if (res) {
        const vec4<T> rr = load4<T>(res + pix + co);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += to_f(rr[k]);
      }
      vec4<T> o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = from_f<T>(p.relu ? fmaxf(v[k], 0.f) : v[k]);
      store4<T>(y + pix + co, o);
    }
  }
}

template <typename T, int TW, int S>
int launch(const Conv3x3Params& p, long long blocks, hipStream_t st) {
  using G = Geo<TW, S>;
  tm_allow_smem(conv3x3_kernel<T, TW, S>, G::SMEM);
  hipLaunchKernelGGL((conv3x3_kernel<T, TW, S>), dim3((unsigned)blocks), dim3(kThreads), G::SMEM, st, p);
  TM_CHECK_LAUNCH();
  return 0;
}

// columns per patch: the power of two in 8..64 that wastes the fewest columns (ties: the widest,
// whose windows carry the least halo)
int pick_tw(int wo) {
  int best = 8;
  long long waste = -1;
  for (int tw = 8; tw <= 64; tw *= 2) {
    const long long cov = (long long)((wo + tw - 1) / tw) * tw;
    if (waste < 0 || cov <= waste) { waste = cov; best = tw; }
  }
  return best;
}

template <typename T, int S>
int dispatch_tw(Conv3x3Params& p, hipStream_t st) {
  const int tw = pick_tw(p.wo);
  const int th = BM / tw;
  p.nseg = (p.wo + tw - 1) / tw;
  p.nct = p.cout / BN;
  const long long blocks = ((p.rows + th - 1) / th) * p.nseg * p.nct;
  TM_REQUIRE(blocks < (1LL << 31), "conv3x3: too many output tiles for one launch (n * ho * wo * cout too large)");
  switch (tw) {
    case 8: return launch<T, 8, S>(p, blocks, st);
    case 16: return launch<T, 16, S>(p, blocks, st);
    case 32: return launch<T, 32, S>(p, blocks, st);
    default: return launch<T, 64, S>(p, blocks, st);
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int tm_conv3x3(int dtype, const void* x, const void* w, const void* bias, const void* residual, void* y,
                          long long n, int h, int wd, int cin, int cout, int stride, int relu, void* stream) {
  TM_REQUIRE(dtype == TM_BF16 || dtype == TM_F32, "conv3x3: dtype must be TM_F32 or TM_BF16");
  TM_REQUIRE(cin >= 64 && cin <= 512 && cin % 64 == 0, "conv3x3: cin must be a multiple of 64 up to 512");
  TM_REQUIRE(cout >= 64 && cout <= 512 && cout % 64 == 0, "conv3x3: cout must be a multiple of 64 up to 512");
  TM_REQUIRE(stride == 1 || stride == 2, "conv3x3: stride must be 1 or 2");
  TM_REQUIRE(h >= 1 && wd >= 1 && h <= kMaxExtent && wd <= kMaxExtent, "conv3x3: h and wd must be in 1..32768");
  TM_REQUIRE(n >= 1 && n < (1LL << 40), "conv3x3: n must be in 1..2^40");
  TM_REQUIRE(x && w && y, "conv3x3: x, w and y must not be NULL");
  TM_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias) && aligned16(residual),
             "conv3x3: pointers must be 16-byte aligned");
  TM_REQUIRE(x != y, "conv3x3: the output must not alias the input");
  Conv3x3Params p;
  p.x = x; p.w = w; p.bias = bias; p.res = residual; p.y = y;
  p.h = h; p.wd = wd; p.ho = (h - 1) / stride + 1; p.wo = (wd - 1) / stride + 1;
  p.rows = n * p.ho;
  p.cin = cin; p.cout = cout; p.relu = relu ? 1 : 0; p.nseg = 0; p.nct = 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_BF16) return stride == 1 ? dispatch_tw<bf16, 1>(p, st) : dispatch_tw<bf16, 2>(p, st);
  return stride == 1 ? dispatch_tw<float, 1>(p, st) : dispatch_tw<float, 2>(p, st);
}
