// Tile-bag ingest from HBM-resident 8-bit tiles (code/datasets/jpg_dataloader.py:229-293): one
// launch gathers, normalises and zero-pads every tile of a batch straight into the encoder's
// compute dtype:
//
//   dst[r][c][h][w] = lut[c][ src[idx[r]][h][w][c] ]      (ToTensor + Normalize, :164-171, as a
//                                                          function of (channel, byte value))
//   dst[r][:][:][:] = 0                                   (idx[r] outside [0, ntiles): the zero
//                                                          tiles of to_fixed_size_bag, :291-292)
//
// The [3][256] fp32 table is computed by the caller with the reference's own torch ops; the kernel
// only rounds it once to the output dtype (into LDS) and looks values up, so its result is bit-equal
// to the elementwise evaluation by construction.  HBM-bound: 3 B read and 2 x 3 / 4 x 3 B written
// per pixel.  Vector path: a lane owns VEC = 16 B / sizeof(T) consecutive pixels of a row (8 in
// bf16, 4 in fp32) = 3 VEC source bytes read as dwords, and writes three 16-B stores -- VEC
// consecutive w of each channel plane (dw == 1: consecutive lanes write consecutive 16-B pieces of a
// plane row, so a wave's store is one contiguous run), or the 3 VEC contiguous elements of a
// channels-last destination (dc == 1, dw == 3).  Everything else (widths that are no multiple of
// VEC, misaligned bases, other strides) takes the pixel-per-lane path, which reads the same table.
// All addressing is 64-bit; the grid is one-dimensional and strides over (tile, 256-lane chunk)
// items, so no count is capped by a grid dimension.
#include "common.h"
#include "../../include/transmil_hip.h"

namespace {

enum { TILES_GENERIC = 0, TILES_PLANES = 1, TILES_PIXELS = 2 };

// one 16-B store of 16 / sizeof(T) consecutive elements (p 16-B aligned)
TM_DEV void store_vec(bf16* p, const bf16* v) {
  bf16x8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = v[j];
  *(bf16x8*)p = a;
}
TM_DEV void store_vec(float* p, const float* v) { *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]}; }

template <typename T, int MODE>
__global__ void __launch_bounds__(256) gather_tiles_kernel(const uint8_t* __restrict__ src, long long ntiles,
                                                           unsigned W, unsigned units, size_t tile_bytes,
                                                           const long long* __restrict__ idx, long long n,
                                                           unsigned cpt, unsigned step_r, unsigned step_c,
                                                           const float* __restrict__ lut, T* __restrict__ dst,
                                                           long long dn, long long dc, long long dh, long long dw) {
  constexpr int VEC = 16 / sizeof(T);      // pixels per lane on the vector paths
  constexpr int NB = 3 * VEC;              // source bytes = output elements per lane
  __shared__ T tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = from_f<T>(lut[i]);
  __syncthreads();
  // item = (output tile r, chunk c of 256 lanes); this block takes items blockIdx.x + k * gridDim.x
  long long r = blockIdx.x / cpt;
  unsigned c = blockIdx.x % cpt;
  for (; r < n; r += step_r, c += step_c) {
    if (c >= cpt) {
      c -= cpt;
      if (++r >= n) break;
    }
    const unsigned u = c * 256 + threadIdx.x;
    if (u >= units) continue;
    const long long t = idx[r];
    const bool pad = t < 0 || t >= ntiles;
    const uint8_t* s = src + (pad ? 0 : (size_t)t * tile_bytes);
    T* d = dst + r * dn;
    if (MODE == TILES_GENERIC) {
      // u = pixel
      const unsigned h = u / W, w = u - h * W;
      d += (long long)h * dh + (long long)w * dw;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        d[ch * dc] = pad ? from_f<T>(0.f) : tab[ch * 256 + s[(size_t)u * 3 + ch]];
      continue;
    }
    // u = group of VEC pixels of one row (W % VEC == 0; s + u * NB is 4-B aligned)
    const unsigned p0 = u * VEC, h = p0 / W, w0 = p0 - h * W;
    unsigned words[NB / 4] = {};
    if (!pad) {
      const unsigned* sw = (const unsigned*)(s + (size_t)u * NB);
#pragma unroll
      for (int k = 0; k < NB / 4; ++k) words[k] = sw[k];
    }
    T out[NB];                             // element e: pixel e / 3, channel e % 3
#pragma unroll
    for (int e = 0; e < NB; ++e) {
      const unsigned byte = (words[e >> 2] >> (8 * (e & 3))) & 0xffu;
      out[e] = pad ? from_f<T>(0.f) : tab[(e % 3) * 256 + byte];
    }
    if (MODE == TILES_PLANES) {
      d += (long long)h * dh + w0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        T plane[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) plane[j] = out[3 * j + ch];
        store_vec(d + ch * dc, plane);
      }
    } else {
      d += (long long)h * dh + (long long)w0 * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) store_vec(d + VEC * k, out + VEC * k);
    }
  }
}

template <typename T>
int launch_tiles(const void* src, long long ntiles, int H, int W, const long long* idx, long long n,
                 const float* lut, void* dst, long long dn, long long dc, long long dh, long long dw,
                 hipStream_t st) {
  constexpr long long VEC = 16 / sizeof(T);
  // W % VEC == 0 makes a tile a multiple of 3 VEC bytes, so every tile base stays 4-B aligned
  const bool src_vec = W % VEC == 0 && ((uintptr_t)src & 3) == 0;
  const bool dst_vec = ((uintptr_t)dst & 15) == 0 && dn % VEC == 0 && dh % VEC == 0;
  int mode = TILES_GENERIC;
  if (src_vec && dst_vec && dw == 1 && dc % VEC == 0) mode = TILES_PLANES;
  else if (src_vec && dst_vec && dc == 1 && dw == 3) mode = TILES_PIXELS;
  const unsigned hw = (unsigned)H * (unsigned)W;
  const unsigned units = mode == TILES_GENERIC ? hw : hw / (unsigned)VEC;
  const unsigned cpt = (units + 255) / 256;
  const long long items = n * (long long)cpt;
  const long long cap = (long long)tm_cu_count() * 32;
  const unsigned grid = (unsigned)(items < cap ? items : cap);
  const unsigned step_r = grid / cpt, step_c = grid % cpt;
  const size_t tile_bytes = (size_t)hw * 3;
#define TM_TILES_LAUNCH(MODE)                                                                              \
  gather_tiles_kernel<T, MODE><<<grid, 256, 0, st>>>((const uint8_t*)src, ntiles, (unsigned)W, units,      \
                                                     tile_bytes, idx, n, cpt, step_r, step_c, lut, (T*)dst, \
                                                     dn, dc, dh, dw)
  if (mode == TILES_PLANES) TM_TILES_LAUNCH(TILES_PLANES);
  else if (mode == TILES_PIXELS) TM_TILES_LAUNCH(TILES_PIXELS);
  else TM_TILES_LAUNCH(TILES_GENERIC);
#undef TM_TILES_LAUNCH
  TM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int tm_gather_tiles_u8(int dtype, const void* src, long long ntiles, int H, int W,
                                  const long long* idx, long long n, const float* lut, void* dst,
                                  long long dn, long long dc, long long dh, long long dw, void* stream) {
  TM_REQUIRE(dtype == TM_F32 || dtype == TM_BF16, "gather_tiles_u8: dtype must be TM_F32 or TM_BF16");
  TM_REQUIRE(src, "gather_tiles_u8: src is null");
  TM_REQUIRE(idx, "gather_tiles_u8: idx is null");
  TM_REQUIRE(lut, "gather_tiles_u8: lut is null");
  TM_REQUIRE(dst, "gather_tiles_u8: dst is null");
  TM_REQUIRE(H > 0 && W > 0, "gather_tiles_u8: H and W must be positive");
  TM_REQUIRE((long long)H * W * 3 < (1ll << 31), "gather_tiles_u8: a tile must be smaller than 2 GiB");
  TM_REQUIRE(ntiles >= 0, "gather_tiles_u8: ntiles must be >= 0");
  TM_REQUIRE(n >= 0, "gather_tiles_u8: n must be >= 0");
  TM_REQUIRE(n < (1ll << 31), "gather_tiles_u8: n must be below 2^31");
  TM_REQUIRE(dn > 0 && dc > 0 && dh > 0 && dw > 0, "gather_tiles_u8: every dst stride must be positive");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TM_F32) return launch_tiles<float>(src, ntiles, H, W, idx, n, lut, dst, dn, dc, dh, dw, st);
  return launch_tiles<bf16>(src, ntiles, H, W, idx, n, lut, dst, dn, dc, dh, dw, st);
}
