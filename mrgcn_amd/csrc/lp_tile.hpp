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

// ---- the bf16 form of the tile ---------------------------------------------------------------------------------------
// x[r][s] = R~[r] . S~[s] on v_mfma_f32_16x16x32_bf16: bf16 operands (a product of two is exact in fp32), fp32 sums, K
// steps of 32.  Lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7, as one
// 16-byte fragment; D is at col = l & 15, row = 4 (l >> 4) + reg — the f32 tile's D map, so the epilogues carry over.
// Both sides arrive as bf16 TABLES (mrgcn_cast_rows_bf16, once per forward): rows of ld % 32 == 0 elements with zeros
// in [H, Hp), Hp = 32 ceil(H / 32), so every load is whole and straight-line with no column clamp.  NK = K steps the
// kernel is built for (Hp / 32 <= NK; the steps past Hp are skipped, block uniform).  The LDS row of a stream tile is
// 32 NK + 8 elements whatever H: 16 NK + 4 dwords, so the 16 rows one ds_read_b128 of the score product touches start
// 4 banks apart (conflict free) and every address below is a compile-time offset from one lane base.
using bf16x8a = __attribute__((ext_vector_type(8))) __bf16;
using s16x4a = __attribute__((ext_vector_type(4))) short;
typedef s16x4a __attribute__((address_space(3))) lds_s16x4a;

constexpr int kBGP = kAT + 8;      // padded row of the bf16 G tile (144 bytes: 16-byte pieces stay aligned)

__host__ __device__ inline int hp32(int H) { return (H + 31) / 32 * 32; }
template <int NK> constexpr int tile_ld() { return 32 * NK + 8; }
template <int NK> constexpr size_t stream_lds_bf16() { return (size_t)kAT * tile_ld<NK>() * sizeof(uint16_t); }
constexpr size_t g_lds_bf16() { return (size_t)kAT * kBGP * sizeof(uint16_t); }

// the wave's 16 rows as the A operand: lane (lm, kq) keeps T[r0 + lm][32 ks + 8 kq .. + 7] for every K step ks (rows
// past the table repeat its last row)
template <int NK>
__device__ __forceinline__ void load_rows_bf16(const uint16_t *__restrict__ T, int64_t ld, int64_t r0, int64_t nrows,
                                               int H, int lm, int kq, bf16x8a (&a)[NK]) {
  const int64_t r = r0 + lm < nrows ? r0 + lm : nrows - 1;
  const uint16_t *row = T + r * ld + 8 * kq;
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    if (32 * ks < H) a[ks] = *reinterpret_cast<const bf16x8a *>(row + 32 * ks);  // block uniform
    else a[ks] = bf16x8a{};
  }
}

// a stream tile: 64 rows of hq = Hp / 8 16-byte pieces; thread t takes pieces t, t + 256, ... (Hp / 32 <= NK of them)
template <int NK>
__device__ __forceinline__ void load_tile_bf16(const uint16_t *__restrict__ T, int64_t ld, int64_t r0, int64_t nrows,
                                               int H, int hq, bf16x8a (&v)[NK]) {
#pragma unroll
  for (int u = 0; u < NK; ++u) {
    if (32 * u < H) {  // block uniform: piece t + 256 u lies inside the 64 rows
      const int i = (int)threadIdx.x + 256 * u;
      const int row = i / hq, k = 8 * (i - row * hq);
      const int64_t r = r0 + row < nrows ? r0 + row : nrows - 1;
      v[u] = *reinterpret_cast<const bf16x8a *>(T + r * ld + k);
    }
  }
}
template <int NK>
__device__ __forceinline__ void store_tile_bf16(uint16_t *__restrict__ Ts, int H, int hq, const bf16x8a (&v)[NK]) {
#pragma unroll
  for (int u = 0; u < NK; ++u) {
    if (32 * u < H) {
      const int i = (int)threadIdx.x + 256 * u;
      const int row = i / hq, k = 8 * (i - row * hq);
      *reinterpret_cast<bf16x8a *>(Ts + row * tile_ld<NK>() + k) = v[u];
    }
  }
}

// acc[j][reg] = row (4 kq + reg of the wave's 16) . stream row (16 j + lm of the tile): four independent accumulators
template <int NK>
__device__ __forceinline__ void score_tile_bf16(const bf16x8a (&a)[NK], const uint16_t *__restrict__ Ts, int H, int lm,
                                                int kq, f32x4a (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4a{0.f, 0.f, 0.f, 0.f};
  const uint16_t *b0 = Ts + lm * tile_ld<NK>() + 8 * kq;
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    if (32 * ks < H) {  // block uniform
      bf16x8a b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8a *>(b0 + 16 * j * tile_ld<NK>() + 32 * ks);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], b[j], acc[j], 0, 0, 0);
    }
  }
}

// the wave's 16 x 64 piece of G, fp32 in D layout, rounded to bf16 ONCE as it becomes the second product's operand:
// lane (lm, kq) writes rows 4 kq + reg, column 16 j + lm of the wave's own LDS rows
__device__ __forceinline__ void store_g_bf16(uint16_t *__restrict__ Gs, int lm, int kq, int j, int reg, float g) {
  reinterpret_cast<__bf16 *>(Gs)[(4 * kq + reg) * kBGP + 16 * j + lm] = (__bf16)g;  // (v_cvt_pk_bf16_f32: nearest even)
}

// the second product: acc2[nt] += G~ (16 x 64, the wave's LDS rows: the A operand read by rows) . S~ (the 64 stream
// rows in LDS, features 16 nt .. 16 nt + 15).  The sum runs over the STREAM rows, so the B operand wants k along the
// rows of the image the score product reads by rows: lane l needs S[32 kk + 8 (l >> 4) + j][16 nt + (l & 15)], j =
// 0..7, which is what two ds_read_b64_tr_b16 deliver from the SAME image — per 16-lane group a block of 4 rows x 16
// columns, lane 4 q + p of the group giving the address of row q, columns 4 p .. 4 p + 3, lane i receiving column i of
// the four rows.  Group g = l >> 4 takes rows 32 kk + 8 g .. + 3 and .. + 4 .. + 7: a 32-lane half's two blocks are 8
// rows apart in the same columns.  All 64 lanes are active here (the ISA requires it) and every address is in bounds.
template <int NK>
__device__ __forceinline__ void second_product_bf16(const uint16_t *__restrict__ Gs, uint16_t *__restrict__ Ss, int H,
                                                    int lm, int kq, f32x4a (&acc2)[2 * NK]) {
  const uint16_t *tb = Ss + (8 * kq + (lm >> 2)) * tile_ld<NK>() + 4 * (lm & 3);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const bf16x8a g = *reinterpret_cast<const bf16x8a *>(Gs + lm * kBGP + 32 * kk + 8 * kq);
#pragma unroll
    for (int nt = 0; nt < 2 * NK; ++nt) {
      if (16 * nt < H) {  // block uniform
        const uint16_t *p = tb + 32 * kk * tile_ld<NK>() + 16 * nt;
        const s16x4a lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4a *)p);
        const s16x4a hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4a *)(p + 4 * tile_ld<NK>()));
        const bf16x8a b = __builtin_bit_cast(bf16x8a, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g, b, acc2[nt], 0, 0, 0);
      }
    }
  }
}

// the shapes the bf16 tile kernels take: bf16 tables of whole K steps, 32-bit row numbers
inline bool shape_ok_bf16(const uint16_t *Q, int64_t ldQ, int64_t m, const uint16_t *E, int64_t ldE, int64_t N,
                          int32_t H) {
  return H % 4 == 0 && H >= 4 && H <= 256 && m >= 1 && N >= 1 && m < ((int64_t)1 << 31) && N < ((int64_t)1 << 31) &&
         ldQ >= hp32(H) && ldE >= hp32(H) && ldQ % 32 == 0 && ldE % 32 == 0 &&
         (((uintptr_t)Q | (uintptr_t)E) & 15) == 0;
}

#define LP_BF16_BY_WIDTH(H, CALL)     \
  ((H) <= 32    ? CALL(1)             \
   : (H) <= 64  ? CALL(2)             \
   : (H) <= 128 ? CALL(4)             \
   : (H) <= 192 ? CALL(6)             \
                : CALL(8))

}  // namespace
}  // namespace mrgcn
