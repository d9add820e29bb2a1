// One labelled row of nn.CrossEntropyLoss()(Y_hat[idx], targets) (node_classification.py:439-444), shared by the loss
// kernels that keep the gradient compact (optim.hip: k_xent_rows; nc_batches.hip: k_nc_xent) so that their gradient
// rows are the same bits by construction: one body, not two that have to be kept in step.
#pragma once

#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace mrgcn {

struct XentRow {
  float lse;  // logf(sum exp(z - max)) + max
  float zt;   // z[t]; 0 for a target outside [0, C), which reads nothing
  int am;     // the arg-max; strict >: of equal values the lowest class stays (Tensor.max(dim=1))
};

using xent_f4 = __attribute__((ext_vector_type(4))) float;

// z: the row's C logits (dword aligned); drow (nullable): the row's C gradient values,
// (expf(z - lse) - onehot(t)) * inv_n.  Max by fmaxf in class order, the exponentials added in class order.
__device__ __forceinline__ XentRow xent_row(const float *__restrict__ z, int C, int64_t t, float inv_n,
                                            float *__restrict__ drow) {
  XentRow r{0.f, 0.f, 0};
  if (C <= 16) {  // the row in registers: all its loads in flight at once (a loop over z[c] waits for each)
    float zz[16];
    if (C >= 4) {
      // four 16-byte pieces per row (dword-aligned addresses: rows may be 44 bytes), each starting inside the row
      // (min(4p, C - 4)) and shifted into place — a quarter of the load instructions of sixteen 4-byte loads: the one
      // block's CU is bound by its address unit when the rows are scattered (10 000 labelled rows: 155 us)
      xent_f4 v[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) v[p] = *reinterpret_cast<const xent_f4 *>(z + (4 * p < C - 4 ? 4 * p : C - 4));
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int shift = 4 * p - (4 * p < C - 4 ? 4 * p : C - 4);  // (wave uniform; > 3: the whole piece lies past C)
        const xent_f4 w = v[p];
        zz[4 * p] = shift == 0 ? w.x : shift == 1 ? w.y : shift == 2 ? w.z : w.w;
        zz[4 * p + 1] = shift == 0 ? w.y : shift == 1 ? w.z : w.w;
        zz[4 * p + 2] = shift == 0 ? w.z : w.w;
        zz[4 * p + 3] = w.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) zz[c] = z[c < C ? c : C - 1];  // (unconditional loads at clamped addresses:
    }                                                             //  a load behind `c < C` waits for itself)
#pragma unroll
    for (int c = 0; c < 16; ++c) zz[c] = c < C ? zz[c] : -INFINITY;
    float mx = zz[0], best = zz[0];
#pragma unroll
    for (int c = 1; c < 16; ++c) {
      mx = fmaxf(mx, zz[c]);
      if (zz[c] > best) {  // (the fill is -inf: never greater)
        best = zz[c];
        r.am = c;
      }
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if (c < C) se += expf(zz[c] - mx);
      if (c == t) r.zt = zz[c];
    }
    r.lse = logf(se) + mx;
    if (drow) {
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < C) drow[c] = (expf(zz[c] - r.lse) - (c == t ? 1.f : 0.f)) * inv_n;
    }
    return r;
  }
  float mx = z[0], best = z[0];
  for (int c = 1; c < C; ++c) {
    const float v = z[c];
    mx = fmaxf(mx, v);
    if (v > best) {
      best = v;
      r.am = c;
    }
  }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
  r.lse = logf(se) + mx;
  if (t >= 0 && t < C) r.zt = z[t];
  if (drow)
    for (int c = 0; c < C; ++c) drow[c] = (expf(z[c] - r.lse) - (c == t ? 1.f : 0.f)) * inv_n;
  return r;
}

}  // namespace mrgcn
