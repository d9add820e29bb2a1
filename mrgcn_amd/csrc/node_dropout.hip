// Node dropout on the device (mrgcn/models/rgcn.py:78-84: one Bernoulli draw per node and layer, the layer's output
// rows scaled by it).
//
//   mrgcn_node_dropout_draw_f32   the masks of one step, drawn with Philox4x32-10 (Salmon et al., SC'11 — the public
//                                 counter-based generator, written out in philox.hpp) from a seed and a stream position that
//                                 live in device memory; the position is advanced by a one-thread launch behind the
//                                 draw, so a replayed hipGraph draws fresh masks on every replay
//   mrgcn_row_scale_f32           Y[r, 0:F] *= m[r] in place on rows with a leading dimension (the forward)
//   mrgcn_row_scale_live_f32      out[r, 0:F] = m[r] * dY[r, 0:F] over the rows a flag byte names (the backward)
//
// All three are one-shot grids of 16-byte accesses: a thread owns one float4 and leaves.
#include "common.hpp"
#include "philox.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;

// ---- the draw (Philox4x32-10: philox.hpp) ----------------------------------------------------------------------------
// One thread draws the four nodes 4g .. 4g+3 of one layer: counter (g, layer, position lo, position hi), key (seed lo,
// seed hi) — a node's value depends on nothing else, whatever the grid.  A node is dropped when its 32-bit word is
// below `threshold` (= floor(p * 2^32): 0 keeps every node, 2^32 drops every node).
__global__ void __launch_bounds__(kTB) k_node_dropout_draw(float *__restrict__ masks, int64_t ld, int64_t n,
                                                           int64_t groups, int32_t layers, int32_t layer0,
                                                           uint64_t threshold, float keep,
                                                           const int64_t *__restrict__ state) {
  const int64_t t = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (t >= groups * layers) return;
  const int32_t l = (int32_t)(t / groups);
  const int64_t g = t - (int64_t)l * groups;
  const uint64_t seed = (uint64_t)state[0], pos = (uint64_t)state[1];
  const U4 r = philox4x32_10(U4{(uint32_t)g, (uint32_t)(layer0 + l), (uint32_t)pos, (uint32_t)(pos >> 32)},
                             (uint32_t)seed, (uint32_t)(seed >> 32));
  float4 v;
  v.x = (uint64_t)r.x < threshold ? 0.f : keep;
  v.y = (uint64_t)r.y < threshold ? 0.f : keep;
  v.z = (uint64_t)r.z < threshold ? 0.f : keep;
  v.w = (uint64_t)r.w < threshold ? 0.f : keep;
  float *row = masks + (int64_t)l * ld;
  const int64_t i = g << 2;
  if (i + 4 <= n) {
    *reinterpret_cast<float4 *>(row + i) = v;   // (ld % 4 == 0 and a 16-byte base: checked by the caller)
  } else {
    if (i < n) row[i] = v.x;
    if (i + 1 < n) row[i + 1] = v.y;
    if (i + 2 < n) row[i + 2] = v.z;
  }
}

__global__ void k_node_dropout_advance(int64_t *__restrict__ state) { state[1] = state[1] + 1; }

// ---- row scale -----------------------------------------------------------------------------------------------------
// rows of whole 16-byte pieces (both leading dimensions % 4 == 0): a thread owns one piece of one row; the columns
// past F of a row's last piece pass through as they are
__global__ void __launch_bounds__(kTB) k_row_scale_pieces(const float *src, int64_t lds, int64_t rows,
                                                          int32_t F, int32_t P, const float *__restrict__ m,
                                                          const uint8_t *__restrict__ flags, int zero_dead,
                                                          float *dst, int64_t ldd) {
  const int64_t t = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (t >= rows * P) return;
  const int64_t r = t / P;
  const int c = (int)(t - r * P) << 2;
  const float s = m[r];
  if (flags && !flags[r]) {
    if (zero_dead) *reinterpret_cast<float4 *>(dst + r * ldd + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float4 v = *reinterpret_cast<const float4 *>(src + r * lds + c);
  v.x *= s;
  if (c + 1 < F) v.y *= s;
  if (c + 2 < F) v.z *= s;
  if (c + 3 < F) v.w *= s;
  *reinterpret_cast<float4 *>(dst + r * ldd + c) = v;
}

// dense rows (both leading dimensions == F): a thread owns four consecutive floats of the flat array, which may lie
// in two rows (or more when F < 4)
__global__ void __launch_bounds__(kTB) k_row_scale_flat(const float *src, int64_t total, int32_t F,
                                                        const float *__restrict__ m,
                                                        const uint8_t *__restrict__ flags, int zero_dead,
                                                        float *dst) {
  const int64_t e = ((int64_t)blockIdx.x * kTB + threadIdx.x) << 2;
  if (e >= total) return;
  float s[4];
  bool live[4];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = (e + j < total ? e + j : total - 1) / F;
    s[j] = m[r];
    live[j] = flags ? flags[r] != 0 : true;
    any |= live[j];
  }
  if (e + 4 <= total) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any) {
      const float4 x = *reinterpret_cast<const float4 *>(src + e);
      v.x = live[0] ? x.x * s[0] : 0.f;   // (select: a dead row of the source may hold anything)
      v.y = live[1] ? x.y * s[1] : 0.f;
      v.z = live[2] ? x.z * s[2] : 0.f;
      v.w = live[3] ? x.w * s[3] : 0.f;
    } else if (!zero_dead) {
      return;
    }
    *reinterpret_cast<float4 *>(dst + e) = v;
  } else {
    for (int j = 0; e + j < total; ++j) {
      if (live[j]) dst[e + j] = src[e + j] * s[j];
      else if (zero_dead) dst[e + j] = 0.f;
    }
  }
}

// any other layout: one float per thread
__global__ void __launch_bounds__(kTB) k_row_scale_scalar(const float *src, int64_t lds, int64_t rows,
                                                          int32_t F, const float *__restrict__ m,
                                                          const uint8_t *__restrict__ flags, int zero_dead,
                                                          float *dst, int64_t ldd) {
  const int64_t t = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (t >= rows * F) return;
  const int64_t r = t / F;
  const int c = (int)(t - r * F);
  if (flags && !flags[r]) {
    if (zero_dead) dst[r * ldd + c] = 0.f;
    return;
  }
  dst[r * ldd + c] = src[r * lds + c] * m[r];
}

int row_scale(const float *src, int64_t lds, int64_t rows, int32_t F, const float *m, const uint8_t *flags,
              int zero_dead, float *dst, int64_t ldd, void *stream) {
  MRGCN_REQUIRE(src && dst && m, "NULL");
  MRGCN_REQUIRE(rows >= 0 && F > 0 && lds >= F && ldd >= F, "F / leading dimensions");
  if (rows == 0) return MRGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  auto blocks = [](int64_t threads) { return dim3((unsigned)((threads + kTB - 1) / kTB)); };
  if (aligned && lds % 4 == 0 && ldd % 4 == 0) {
    const int32_t P = (F + 3) / 4;
    MRGCN_REQUIRE(rows * P < ((int64_t)1 << 31) * kTB, "too many rows for one grid");
    k_row_scale_pieces<<<blocks(rows * P), dim3(kTB), 0, st>>>(src, lds, rows, F, P, m, flags, zero_dead, dst, ldd);
  } else if (aligned && lds == F && ldd == F) {
    const int64_t total = rows * (int64_t)F;
    MRGCN_REQUIRE((total + 3) / 4 < ((int64_t)1 << 31) * kTB, "too many rows for one grid");
    k_row_scale_flat<<<blocks((total + 3) / 4), dim3(kTB), 0, st>>>(src, total, F, m, flags, zero_dead, dst);
  } else {
    MRGCN_REQUIRE(rows * F < ((int64_t)1 << 31) * kTB, "too many rows for one grid");
    k_row_scale_scalar<<<blocks(rows * F), dim3(kTB), 0, st>>>(src, lds, rows, F, m, flags, zero_dead, dst, ldd);
  }
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // namespace

int philox_state_advance(int64_t *state_dev, hipStream_t s) {
  k_node_dropout_advance<<<dim3(1), dim3(1), 0, s>>>(state_dev);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}
}  // namespace mrgcn

extern "C" {

int mrgcn_node_dropout_draw_f32(float *masks, int64_t ld, int64_t n, int32_t layers, int32_t layer0,
                                int64_t threshold, float keep_value, int64_t *state_dev, int32_t advance,
                                void *stream) {
  MRGCN_REQUIRE(masks && state_dev, "NULL");
  MRGCN_REQUIRE(n >= 0 && n <= ((int64_t)1 << 32) && layers >= 1 && layer0 >= 0, "n / layers");
  MRGCN_REQUIRE(ld >= n && (layers == 1 || ld % 4 == 0) && ((uintptr_t)masks & 15) == 0,
                "masks: rows of whole 16-byte pieces on a 16-byte base");
  MRGCN_REQUIRE(threshold >= 0 && threshold <= ((int64_t)1 << 32), "threshold is floor(p * 2^32)");
  hipStream_t st = (hipStream_t)stream;
  const int64_t groups = (n + 3) / 4;
  if (groups > 0) {
    const int64_t threads = groups * layers;
    mrgcn::k_node_dropout_draw<<<dim3((unsigned)((threads + mrgcn::kTB - 1) / mrgcn::kTB)), dim3(mrgcn::kTB), 0, st>>>(
        masks, ld, n, groups, layers, layer0, (uint64_t)threshold, keep_value, state_dev);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  if (advance) {
    mrgcn::k_node_dropout_advance<<<dim3(1), dim3(1), 0, st>>>(state_dev);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  return MRGCN_OK;
}

int mrgcn_row_scale_f32(float *Y, int64_t ld, int64_t rows, int32_t F, const float *m, void *stream) {
  return mrgcn::row_scale(Y, ld, rows, F, m, nullptr, 0, Y, ld, stream);
}

int mrgcn_row_scale_live_f32(const float *dY, int64_t ld_dY, int64_t rows, int32_t F, const float *m,
                             const uint8_t *row_flags, int32_t zero_dead, float *out, int64_t ld_out, void *stream) {
  return mrgcn::row_scale(dY, ld_dY, rows, F, m, row_flags, zero_dead, out, ld_out, stream);
}

}  // extern "C"
