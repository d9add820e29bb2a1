// The 64 x 64 score tile of the all-candidates decoders (lp_all.hip: the 1-vs-all softmax; lp_kvsall.hip: the KvsAll
// BCE): x[r][s] = R[r] . S[s] on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32; lane maps as basis_xform.hip's
// k_bx_gemm), consumed in registers.  The ROW side (64 rows, 16 per wave) sits in registers as the A operand for the
// whole kernel, the STREAM side passes through LDS 64 rows at a time as the B operand; the next tile's rows are loaded
// into registers while the present one is multiplied.  Every load is straight-line at a clamped position; what a
// padded row or column holds is masked out of every sum by the kernel that consumes the tile.
#pragma once

#include "common.hpp"

#include <cmath>

namespace mrgcn {
namespace {

using f32x4a = __attribute__((ext_vector_type(4))) float;

constexpr int kAT = 64;            // rows of a tile on either side
constexpr int kAGP = kAT + 4;      // padded row of the G tile
constexpr int kAllChunk = 1024;    // candidates per forward chunk (a multiple of kAT)
constexpr int kSplitTiles = 256;   // fewer query tiles than this: the forward splits the candidates over gridDim.y
constexpr int kMergeTB = 256;

inline int hp16(int H) { return (H + 15) / 16 * 16; }
inline size_t stream_lds(int H) { return (size_t)kAT * (hp16(H) + 4) * sizeof(float); }
inline int64_t chunk_of(int64_t m, int64_t N) {  // candidates per forward chunk; N: no split
  if ((m + kAT - 1) / kAT >= kSplitTiles) return N;
  int64_t c = kAllChunk;
  const int64_t n = (N + c - 1) / c;
  if (n > 65535) c *= (n + 65534) / 65535;
  return c;
}
inline int64_t chunks_of(int64_t m, int64_t N) {
  const int64_t c = chunk_of(m, N);
  return (N + c - 1) / c;
}
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// the wave's 16 rows of a table as the A operand: lane (lm, kq) keeps T[r0 + lm][16 ks + 4 kq .. + 3] for every K step
// ks (zero past H; rows past the table repeat its last row)
template <int NT>
__device__ __forceinline__ void load_rows(const float *__restrict__ T, int64_t ld, int64_t r0, int64_t nrows, int H,
                                          int lm, int kq, f32x4a (&a)[4 * NT]) {
  const int64_t r = r0 + lm < nrows ? r0 + lm : nrows - 1;
  const float *row = T + r * ld;
#pragma unroll
  for (int ks = 0; ks < 4 * NT; ++ks) {
    const int k = 16 * ks + 4 * kq;
    const f32x4a v = *reinterpret_cast<const f32x4a *>(row + (k < H ? k : H - 4));
    a[ks] = k < H ? v : f32x4a{0.f, 0.f, 0.f, 0.f};
  }
}

// a stream tile: 64 rows of hq = hp16(H) / 4 16-byte pieces; thread t takes pieces t, t + 256, ... (4 NT at most)
template <int NT>
__device__ __forceinline__ void load_tile(const float *__restrict__ T, int64_t ld, int64_t r0, int64_t nrows, int H,
                                          int hq, f32x4a (&v)[4 * NT]) {
#pragma unroll
  for (int u = 0; u < 4 * NT; ++u) {
    const int i = (int)threadIdx.x + 256 * u;
    int row = i / hq;
    const int k = 4 * (i - row * hq);
    row = row < kAT ? row : kAT - 1;
    const int64_t r = r0 + row < nrows ? r0 + row : nrows - 1;
    const f32x4a x = *reinterpret_cast<const f32x4a *>(T + r * ld + (k < H ? k : H - 4));
    v[u] = k < H ? x : f32x4a{0.f, 0.f, 0.f, 0.f};
  }
}
template <int NT>
__device__ __forceinline__ void store_tile(float *__restrict__ Ts, int lds, int hq, const f32x4a (&v)[4 * NT]) {
#pragma unroll
  for (int u = 0; u < 4 * NT; ++u) {
    const int i = (int)threadIdx.x + 256 * u;
    const int row = i / hq, k = 4 * (i - row * hq);
    if (row < kAT) *reinterpret_cast<f32x4a *>(Ts + row * lds + k) = v[u];
  }
}

// acc[j][reg] = row (4 kq + reg of the wave's 16) . stream row (16 j + lm of the tile): four independent accumulators
template <int NT>
__device__ __forceinline__ void score_tile(const f32x4a (&a)[4 * NT], const float *__restrict__ Ts, int lds, int H,
                                           int lm, int kq, f32x4a (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4a{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4 * NT; ++ks) {
    if (16 * ks < H) {  // block uniform
      f32x4a b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4a *>(Ts + (16 * j + lm) * lds + 16 * ks + 4 * kq);
      // k slot kq of the s-th MFMA stands for k = 16 ks + 4 kq + s
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks].x, b[j].x, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks].y, b[j].y, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks].z, b[j].z, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks].w, b[j].w, acc[j], 0, 0, 0);
    }
  }
}

// over the 16 lanes that hold one row of a D tile (lane & 15 = the column)
__device__ __forceinline__ float row_max(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, kWave));
  return x;
}
__device__ __forceinline__ float row_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

// the shapes the tile kernels take: whole 16-byte pieces, at most four K tiles of 64, 32-bit row numbers
inline bool shape_ok(const float *Q, int64_t ldQ, int64_t m, const float *E, int64_t ldE, int64_t N, int32_t H) {
  return H % 4 == 0 && H >= 4 && H <= 256 && m >= 1 && N >= 1 && m < ((int64_t)1 << 31) && N < ((int64_t)1 << 31) &&
         ldQ >= H && ldE >= H && ldQ % 4 == 0 && ldE % 4 == 0 && (((uintptr_t)Q | (uintptr_t)E) & 15) == 0;
}

#define LP_ALL_BY_WIDTH(H, CALL)      \
  ((H) <= 64    ? CALL(1)             \
   : (H) <= 128 ? CALL(2)             \
   : (H) <= 192 ? CALL(3)             \
                : CALL(4))

}  // namespace
}  // namespace mrgcn
