// Type-constrained ranks (Krompass, Baier, Tresp: "Type-Constrained Representation Learning in Knowledge Graphs", ISWC
// 2015): a fact (s, p, o) is ranked against the nodes that can stand in the corrupted place — slot 2 p of a CSR over
// 2 R node lists (the relation's tails: its range) for the tail side, slot 2 p + 1 (its heads: its domain) for the
// head side — instead of against every node of the graph (lp_eval.hip: mrgcn_distmult_ranks_both).
//   truth    the fact's own score, k_truth_both's arithmetic (per side for ComplEx); every fact is scored — the
//            reference's "position >= num_nodes is unscored" belongs to compute_ranks_fast and is not carried over
//   counts   a block owns ONE work item: a fact tile (at most kLpFB facts of one relation, the host's grouping), a side
//            and a tile of kLpTB list positions.  Thread t takes candidate c = idx[slot begin + position] and calls
//            lp_score_tile<SC> with that c: the same float32 operations in the same order as the untyped kernels, so a
//            candidate's score has compute_ranks_fast's bits.  The counts go through LDS as in k_rank_counts_both.
//   final    lp_rank_of over the counts, in the caller's fact order.
// The grid is a work list, not a rectangle: slot lengths of real graphs are skewed (a literal relation's range against
// `type`'s), and a rectangle sized by the longest slot would be mostly blocks that leave at once.
#include "common.hpp"
#include "lp_score.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = kLpTB;
constexpr int kFB = kLpFB;
constexpr int kHT = kLpHT;

// truth[f] (tail side's operations) and, for ComplEx, truth[nf + f] (head side's); counts[8 f ..] = 0
template <int SC>
__global__ void k_typed_truth(const float *__restrict__ E, int64_t ldE, const float *__restrict__ Rel, int64_t ldR,
                              int H, const int64_t *__restrict__ tr, int64_t nf, float *__restrict__ truth,
                              int32_t *__restrict__ counts) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) counts[8 * f + k] = 0;
  const int64_t si = tr[3 * f], pi = tr[3 * f + 1], oi = tr[3 * f + 2];
  const float *s = E + si * ldE, *o = E + oi * ldE;
  float acc = 0.f;
  if constexpr (SC == kLpComplEx) {
    float acc_h = 0.f;
    for (int h = 0; h < H; ++h) {
      float qt, qh, unused;
      lp_stage<SC>(E, ldE, Rel, ldR, H, false, si, pi, h, qt, unused);
      lp_stage<SC>(E, ldE, Rel, ldR, H, true, oi, pi, h, qh, unused);
      const float pt = qt * o[h];
      const float ph = qh * s[h];
      acc = acc + pt;
      acc_h = acc_h + ph;
    }
    truth[nf + f] = acc_h;
  } else {
    const float *p = Rel + pi * ldR;
    for (int h = 0; h < H; ++h) {
      const float sp = s[h] * p[h];
      const float spo = sp * o[h];
      acc = acc + spo;
    }
  }
  truth[f] = acc;
}

// One block per work item {2 tile + side, candidate tile}.  counts[8 f + 4 side + w] as in lp_eval.hip: w = 0 greater,
// 1 ties, 2 masked and greater, 3 masked and tie; f is the fact's index in the caller's order (order[]).
template <int SC>
__global__ __launch_bounds__(kTB) void k_typed_rank_counts(
    const float *__restrict__ Et, int64_t N, int H, const float *__restrict__ E, int64_t ldE,
    const float *__restrict__ Rel, int64_t ldR, const int64_t *__restrict__ tr, int64_t nf,
    const int64_t *__restrict__ order, const int64_t *__restrict__ tile_ptr, const int32_t *__restrict__ tile_rel,
    int64_t ntiles, const int32_t *__restrict__ work, const int64_t *__restrict__ cand_ptr,
    const int32_t *__restrict__ cand_idx, const float *__restrict__ truth, const int64_t *__restrict__ tail_ptr,
    const int32_t *__restrict__ tail_idx, const int64_t *__restrict__ head_ptr, const int32_t *__restrict__ head_idx,
    int32_t *__restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ float s_a[kFB][kHT];
  __shared__ float s_b[kFB][kHT];
  __shared__ int s_cnt[kFB][4];
  const int32_t w0 = work[2 * (int64_t)blockIdx.x], ctile = work[2 * (int64_t)blockIdx.x + 1];
  const bool head = (w0 & 1) != 0;
  const int64_t tile = w0 >> 1;
  if (tile < 0 || tile >= ntiles || ctile < 0) return;      // (block-uniform, before any barrier)
  const int64_t p0 = tile_ptr[tile];
  int64_t cnt = tile_ptr[tile + 1] - p0;
  if (p0 < 0 || cnt <= 0 || p0 + cnt > nf) return;
  const int nfb = (int)(cnt < kFB ? cnt : kFB);
  const int64_t slot = 2 * (int64_t)tile_rel[tile] + (head ? 1 : 0);
  const int64_t begin = cand_ptr[slot], len = cand_ptr[slot + 1] - begin;
  const int64_t pos = (int64_t)ctile * kTB + threadIdx.x;
  const bool live = pos < len;
  int64_t c = live ? (int64_t)cand_idx[begin + pos] : 0;
  c = c < 0 ? 0 : c >= N ? N - 1 : c;                       // (ids are the caller's contract; never a read past Et)
  float acc[kFB];
  if (threadIdx.x < kFB * 4) s_cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;
  lp_score_tile<SC>(Et, N, H, E, ldE, Rel, ldR, head, c, live, nfb,
                    [&](int fi, int64_t &anchor, int64_t &rel) {
                      const int64_t f = order[p0 + fi];
                      anchor = tr[3 * f + (head ? 2 : 0)];
                      rel = tr[3 * f + 1];
                    },
                    s_a, s_b, acc);
  const int64_t *fptr = head ? head_ptr : tail_ptr;
  const int32_t *fidx = head ? head_idx : tail_idx;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kFB; ++i) {
    bool gt = false, eq = false, masked = false;
    if (i < nfb && live) {
      const int64_t f = order[p0 + i];
      const float t = truth[(SC == kLpComplEx && head ? nf : 0) + f];
      gt = acc[i] > t;
      eq = acc[i] == t;
      if (fptr && (gt || eq)) masked = in_sorted(fidx, fptr[f], fptr[f + 1], (int32_t)c);
    }
    const int ngt = __popcll(__ballot(gt)), neq = __popcll(__ballot(eq));
    int nmgt = 0, nmeq = 0;
    if (fptr) {
      nmgt = __popcll(__ballot(gt && masked));
      nmeq = __popcll(__ballot(eq && masked));
    }
    if (lane == 0) {
      if (ngt) atomicAdd(&s_cnt[i][0], ngt);
      if (neq) atomicAdd(&s_cnt[i][1], neq);
      if (nmgt) atomicAdd(&s_cnt[i][2], nmgt);
      if (nmeq) atomicAdd(&s_cnt[i][3], nmeq);
    }
  }
  __syncthreads();
  if (threadIdx.x < nfb * 4) {
    const int i = threadIdx.x >> 2, w = threadIdx.x & 3;
    const int v = s_cnt[i][w];
    if (v) atomicAdd(&counts[8 * order[p0 + i] + (head ? 4 : 0) + w], v);
  }
}

__global__ void k_typed_rank_final(const int32_t *__restrict__ counts, int64_t nf, int64_t *__restrict__ raw,
                                   int64_t *__restrict__ flt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * nf) return;
  const bool head = i >= nf;
  const int32_t *cn = counts + 8 * (head ? i - nf : i) + (head ? 4 : 0);
  const int64_t gt = cn[0], eq = cn[1] > 0 ? cn[1] : 1;   // (the fact's own answer is in its slot: the host checks)
  raw[i] = lp_rank_of(gt, eq);
  if (flt) flt[i] = lp_rank_of(gt - cn[2], eq - cn[3]);
}

// Et [H, N] floats | truth [sides nf] floats | counts [8 nf] int32
inline int64_t typed_ranks_bytes(int64_t num_nodes, int32_t H, int64_t num_facts, int sides) {
  if (num_nodes <= 0 || H <= 0 || num_facts < 0) return -1;
  return (int64_t)sizeof(float) * ((int64_t)H * num_nodes + sides * num_facts) +
         (int64_t)sizeof(int32_t) * 8 * num_facts;
}

template <int SC>
int typed_ranks_run(const char *who_, const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR,
                    int32_t H, const int64_t *triples, int64_t num_facts, const int64_t *order,
                    const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                    int64_t num_work, const int64_t *cand_ptr, const int32_t *cand_idx, const int64_t *tail_ptr,
                    const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx, void *workspace,
                    int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt, void *stream) {
  const std::string who(who_);
  constexpr int kSides = SC == kLpComplEx ? 2 : 1;
  MRGCN_REQUIRE(E && Rel && triples && ranks_raw && workspace && H > 0 && num_nodes > 0 &&
                    num_nodes < ((int64_t)1 << 31) && num_facts >= 0,
                who + ": bad argument");
  MRGCN_REQUIRE(order && tile_ptr && tile_rel && cand_ptr && cand_idx && num_tiles >= 0 && num_work >= 0 &&
                    num_work < ((int64_t)1 << 31) && num_tiles < ((int64_t)1 << 30) && (work || num_work == 0),
                who + ": grouping (order, tile_ptr, tile_rel, work) and candidate lists (cand_ptr, cand_idx)");
  MRGCN_REQUIRE((tail_ptr == nullptr) == (head_ptr == nullptr) && (tail_ptr == nullptr) == (tail_idx == nullptr) &&
                    (head_ptr == nullptr) == (head_idx == nullptr),
                who + ": give all four filter arrays or none");
  MRGCN_REQUIRE(tail_ptr == nullptr || ranks_flt != nullptr, who + ": filter lists without ranks_flt");
  MRGCN_REQUIRE(workspace_bytes >= typed_ranks_bytes(num_nodes, H, num_facts, kSides), who + ": workspace too small");
  if (num_facts == 0) return MRGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  float *Et = (float *)workspace;
  float *truth = Et + (int64_t)H * num_nodes;
  int32_t *counts = (int32_t *)(truth + kSides * num_facts);
  MRGCN_HIP_TRY(lp_transpose(E, ldE, num_nodes, H, Et, st));
  k_typed_truth<SC><<<(unsigned)((num_facts + 127) / 128), 128, 0, st>>>(E, ldE, Rel, ldR, H, triples, num_facts,
                                                                          truth, counts);
  MRGCN_HIP_TRY(hipGetLastError());
  if (num_work > 0) {
    k_typed_rank_counts<SC><<<(unsigned)num_work, kTB, 0, st>>>(Et, num_nodes, H, E, ldE, Rel, ldR, triples, num_facts,
                                                                order, tile_ptr, tile_rel, num_tiles, work, cand_ptr,
                                                                cand_idx, truth, tail_ptr, tail_idx, head_ptr, head_idx,
                                                                counts);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  k_typed_rank_final<<<(unsigned)((2 * num_facts + 255) / 256), 256, 0, st>>>(counts, num_facts, ranks_raw,
                                                                             tail_ptr ? ranks_flt : nullptr);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int64_t mrgcn_distmult_typed_ranks_workspace(int64_t num_nodes, int32_t H, int64_t num_facts) {
  return typed_ranks_bytes(num_nodes, H, num_facts, 1);
}

int mrgcn_distmult_typed_ranks(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                               const int64_t *triples, int64_t num_facts, const int64_t *order,
                               const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                               int64_t num_work, const int64_t *cand_ptr, const int32_t *cand_idx,
                               const int64_t *tail_ptr, const int32_t *tail_idx, const int64_t *head_ptr,
                               const int32_t *head_idx, void *workspace, int64_t workspace_bytes, int64_t *ranks_raw,
                               int64_t *ranks_flt, void *stream) {
  return typed_ranks_run<kLpDistMult>("distmult_typed_ranks", E, ldE, num_nodes, Rel, ldR, H, triples, num_facts, order,
                                      tile_ptr, tile_rel, num_tiles, work, num_work, cand_ptr, cand_idx, tail_ptr,
                                      tail_idx, head_ptr, head_idx, workspace, workspace_bytes, ranks_raw, ranks_flt,
                                      stream);
}

int64_t mrgcn_complex_typed_ranks_workspace(int64_t num_nodes, int32_t H, int64_t num_facts) {
  return H % 2 == 0 ? typed_ranks_bytes(num_nodes, H, num_facts, 2) : -1;
}

int mrgcn_complex_typed_ranks(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *order,
                              const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                              int64_t num_work, const int64_t *cand_ptr, const int32_t *cand_idx,
                              const int64_t *tail_ptr, const int32_t *tail_idx, const int64_t *head_ptr,
                              const int32_t *head_idx, void *workspace, int64_t workspace_bytes, int64_t *ranks_raw,
                              int64_t *ranks_flt, void *stream) {
  MRGCN_REQUIRE(H > 0 && H % 2 == 0, "complex_typed_ranks: H must be even (H / 2 complex numbers per row)");
  return typed_ranks_run<kLpComplEx>("complex_typed_ranks", E, ldE, num_nodes, Rel, ldR, H, triples, num_facts, order,
                                     tile_ptr, tile_rel, num_tiles, work, num_work, cand_ptr, cand_idx, tail_ptr,
                                     tail_idx, head_ptr, head_idx, workspace, workspace_bytes, ranks_raw, ranks_flt,
                                     stream);
}

}  // extern "C"
