// Edge dropout on the device (Schlichtkrull et al. 2018, §5: rate 0.4 on ordinary edges, 0.2 on self-loops, drawn anew
// every step; Rong et al. 2020, DropEdge).
//
//   mrgcn_edge_dropout_draw_f32   rewrites the three value arrays of a value overlay (plan.hip: create_overlay) from its
//                                 parent's: entry (row i, source node j, relation r) of layer l is dropped when word x of
//                                 Philox4x32-10 (philox.hpp) with counter (i, j, r | l << 24, position lo) and key
//                                 (seed lo, seed hi ^ position hi ^ kEdgeTag) is below floor(p_r * 2^32), and holds
//                                 a * keep_r otherwise (keep_r = 1 / (1 - p_r) in fp32, or 1 without rescaling)
//
// The draw is keyed by the entry's COORDINATES, not by its number in some order: the literal CSR (val), the compact view
// (mval) and the CSC (cval) store the entries in three orders, and each pass recovers (i, j, r) from the index arrays of
// its own order — so the three copies agree without a sort, a permutation array or a host round trip, and the result
// depends on nothing but (seed, position, layer, i, j, r, p_r).  Seed and position live in device memory ({seed,
// position}, the pair node dropout uses); a one-thread launch behind the last layer's draw moves the position, so a
// replayed hipGraph draws fresh values on every replay.
//
// Three one-shot grids (a thread owns four consecutive entries and leaves): 16-byte loads of the rows, the columns and
// the parent's values, one 16-byte store.  ~16 bytes per entry and pass.
#include "common.hpp"
#include "philox.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;
constexpr uint32_t kEdgeTag = 0x45444745u;  // "EDGE": another stream than node dropout's and the negatives' under one seed

struct DrawKey {
  uint32_t k0, k1, pos_lo, layer_bits;
};

// COLS_ARE_COMPACT: `cols` holds compact column ids (the CSC pass: ecol), their literal column is ulcol[c]; otherwise
// `cols` holds literal columns r * N + j themselves (lcol / mlcol)
__device__ __forceinline__ float draw_one(int32_t row, uint32_t lc, float a, uint32_t N, const float *__restrict__ rates,
                                          int rescale, const DrawKey &k) {
  const uint32_t r = lc / N, j = lc - r * N;
  const float p = rates[r];
  if (!(p > 0.f)) return a;   // (rate 0: the parent's bits)
  // floor(p * 2^32): the product is exact in fp32 (a power of two), the conversion truncates
  const uint64_t thr = p >= 1.f ? ((uint64_t)1 << 32) : (uint64_t)(p * 4294967296.0f);
  const U4 w = philox4x32_10(U4{(uint32_t)row, j, r | k.layer_bits, k.pos_lo}, k.k0, k.k1);
  if ((uint64_t)w.x < thr) return 0.f;
  return rescale ? a * (1.0f / (1.0f - p)) : a;
}

template <bool COLS_ARE_COMPACT>
__global__ void __launch_bounds__(kTB) k_edge_dropout_draw(const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ cols,
                                                           const int32_t *__restrict__ ulcol,
                                                           const float *__restrict__ src, float *__restrict__ dst,
                                                           int64_t nnz, uint32_t N, const float *__restrict__ rates,
                                                           int rescale, uint32_t layer,
                                                           const int64_t *__restrict__ state) {
  const int64_t e = ((int64_t)blockIdx.x * kTB + threadIdx.x) << 2;
  if (e >= nnz) return;
  const uint64_t seed = (uint64_t)state[0], pos = (uint64_t)state[1];
  DrawKey k;
  k.k0 = (uint32_t)seed;
  k.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(pos >> 32) ^ kEdgeTag;
  k.pos_lo = (uint32_t)pos;
  k.layer_bits = layer << 24;
  if (e + 4 <= nnz) {   // (every array is a pool block: 256-byte bases, so piece e / 4 is 16-byte aligned)
    const int4 ri = *reinterpret_cast<const int4 *>(rows + e);
    int4 ci = *reinterpret_cast<const int4 *>(cols + e);
    const float4 a = *reinterpret_cast<const float4 *>(src + e);
    if (COLS_ARE_COMPACT) {
      ci.x = ulcol[ci.x];
      ci.y = ulcol[ci.y];
      ci.z = ulcol[ci.z];
      ci.w = ulcol[ci.w];
    }
    float4 v;
    v.x = draw_one(ri.x, (uint32_t)ci.x, a.x, N, rates, rescale, k);
    v.y = draw_one(ri.y, (uint32_t)ci.y, a.y, N, rates, rescale, k);
    v.z = draw_one(ri.z, (uint32_t)ci.z, a.z, N, rates, rescale, k);
    v.w = draw_one(ri.w, (uint32_t)ci.w, a.w, N, rates, rescale, k);
    *reinterpret_cast<float4 *>(dst + e) = v;
  } else {
    for (int64_t q = e; q < nnz; ++q) {
      int32_t c = cols[q];
      if (COLS_ARE_COMPACT) c = ulcol[c];
      dst[q] = draw_one(rows[q], (uint32_t)c, src[q], N, rates, rescale, k);
    }
  }
}

}  // namespace
}  // namespace mrgcn

extern "C" {

int mrgcn_edge_dropout_draw_f32(mrgcn_plan_t *child, const float *rates, int32_t rescale, int64_t *state_dev,
                                int32_t layer, int32_t advance, void *stream) {
  using namespace mrgcn;
  MRGCN_REQUIRE(child && rates && state_dev, "NULL");
  const mrgcn_plan *par = child->parent;
  MRGCN_REQUIRE(par != nullptr, "edge dropout draws into a value overlay (mrgcn_plan_create_overlay), not into a plan");
  MRGCN_REQUIRE(child->num_relations < ((int64_t)1 << 24), "edge dropout: fewer than 2^24 relations (the key packs r | layer << 24)");
  MRGCN_REQUIRE(layer >= 0 && layer < 256, "edge dropout: layer 0 .. 255 (the key packs r | layer << 24)");
  MRGCN_REQUIRE((((uintptr_t)child->val | (uintptr_t)child->mval | (uintptr_t)child->cval | (uintptr_t)par->val |
                  (uintptr_t)par->mval | (uintptr_t)par->cval) & 15) == 0, "value arrays on 16-byte bases");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nnz = child->nnz;
  if (nnz > 0) {
    MRGCN_REQUIRE(par->ecol && (par->lean || (par->mlcol && par->mrow)), "edge dropout: the parent's entry coordinates are missing");
    const dim3 grid((unsigned)(((nnz + 3) / 4 + kTB - 1) / kTB)), block(kTB);
    const uint32_t N = (uint32_t)child->num_nodes;
    // the literal CSR: row of every entry (rowidx), literal column (lcol)
    k_edge_dropout_draw<false><<<grid, block, 0, s>>>(par->rowidx, par->lcol, nullptr, par->val, child->val, nnz, N, rates,
                                                      rescale, (uint32_t)layer, state_dev);
    // the compact view: row by rank (mrow), literal column of the operand row (mlcol); a lean plan's is its CSR
    if (!par->lean)
      k_edge_dropout_draw<false><<<grid, block, 0, s>>>(par->mrow, par->mlcol, nullptr, par->mval, child->mval, nnz, N,
                                                        rates, rescale, (uint32_t)layer, state_dev);
    // the CSC: row (crow), compact column (ecol) -> literal column (ulcol)
    k_edge_dropout_draw<true><<<grid, block, 0, s>>>(par->crow, par->ecol, par->ulcol, par->cval, child->cval, nnz, N,
                                                     rates, rescale, (uint32_t)layer, state_dev);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  if (advance) return philox_state_advance(state_dev, s);
  return MRGCN_OK;
}

}  // extern "C"
