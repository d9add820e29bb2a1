// Mini-batch link prediction on fixed batches (mrgcn_amd.tasks.link_prediction: batch_eval, eval_batches, rank_batches,
// fit_batches): what test_model (tasks/link_prediction.py:375-422) takes from ONE batch — raw and filtered ranks of the
// batch's facts against the batch's own few-hundred-row embedding table, and the batch's eight metric values — in three
// launches, and the epoch's row as the unweighted means over the batches' slots (:331, :416-419).  Stream ordered,
// allocation free, no float atomics: a hipGraph replays an epoch of them and equal inputs give equal bits.
//   prep     Et = E^T and the facts' true scores in one grid (transpose tiles, then truth blocks)
//   ranks    a block OWNS eight facts of one direction across all candidate tiles, up to four candidates per thread at
//            once: the scores are lp_score_tiles' (lp_score.hpp: lp_score_tile's operations, the body
//            mrgcn_distmult_ranks runs), the four counts of a fact stay in LDS as integers and the block writes its own
//            raw and filtered ranks — no global counts, no zeroing, no final pass
//   metrics  one wave per rank type, in mrgcn_rank_metrics' order for one part
#include "common.hpp"
#include "lp_score.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = kLpTB;
constexpr int kFB = kLpFB;
constexpr int kHT = kLpHT;
constexpr int kTruthFacts = 256;   // facts per truth block of the prep grid

// blocks [0, ttiles): Et[h, c] = E[c, h], 32 x 32 tiles (tiles_c of them per row of tiles); blocks behind them:
// truth[f] as k_true_scores writes it — sum_h (E[s,h] Rel[p,h]) E[o,h], sequential, nothing contracted; 0 for the facts
// at positions >= N, which the reference never scores (link_prediction.py:611-625)
__global__ __launch_bounds__(256) void k_batch_prep(const float *__restrict__ E, int64_t ldE, int64_t N, int H,
                                                    const float *__restrict__ Rel, int64_t ldR,
                                                    const int64_t *__restrict__ tr, int64_t nf, int64_t tiles_c,
                                                    int64_t ttiles, float *__restrict__ Et,
                                                    float *__restrict__ truth) {
#pragma clang fp contract(off)
  __shared__ float tile[32][33];
  const int64_t b = blockIdx.x;
  if (b < ttiles) {
    const int64_t c0 = (b % tiles_c) * 32;
    const int h0 = (int)(b / tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
      const int64_t c = c0 + r;
      const int h = h0 + tx;
      tile[r][tx] = (c < N && h < H) ? E[c * ldE + h] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int h = h0 + r;
      const int64_t c = c0 + tx;
      if (h < H && c < N) Et[(int64_t)h * N + c] = tile[tx][r];
    }
    return;
  }
  const int64_t f = (b - ttiles) * kTruthFacts + threadIdx.x;
  if (f >= nf) return;
  float acc = 0.f;
  if (f < N) {
    const float *s = E + tr[3 * f] * ldE, *p = Rel + tr[3 * f + 1] * ldR, *o = E + tr[3 * f + 2] * ldE;
    for (int h = 0; h < H; ++h) {
      const float sp = s[h] * p[h];
      const float spo = sp * o[h];
      acc = acc + spo;
    }
  }
  truth[f] = acc;
}

// grid (fact tiles, 2 directions).  s_cnt[i][w], w: 0 greater, 1 ties (all live candidates), 2 masked and greater,
// 3 masked and tie — lp_eval.hip's four counts; the filtered counts are (0) - (2) and (1) - (3).  A thread scores CT
// candidates at once (lp_score_tiles: the pairs' vectors are staged and read once for all of them); a table of more
// than CT tiles takes the loop again.
template <int CT>
__global__ __launch_bounds__(kTB) void k_batch_ranks(
    const float *__restrict__ Et, int64_t N, int H, const float *__restrict__ E, int64_t ldE,
    const float *__restrict__ Rel, int64_t ldR, const int64_t *__restrict__ tr, int64_t nf,
    const float *__restrict__ truth, const int64_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_idx,
    const int64_t *__restrict__ head_ptr, const int32_t *__restrict__ head_idx, int64_t *__restrict__ raw,
    int64_t *__restrict__ flt) {
#pragma clang fp contract(off)
  __shared__ float s_a[kFB][kHT];
  __shared__ float s_b[kFB][kHT];
  __shared__ int s_cnt[kFB][4];
  const bool head = blockIdx.y == 1;
  const int64_t f0 = (int64_t)blockIdx.x * kFB;
  const int nfb = (int)((nf - f0) < kFB ? (nf - f0) : kFB);
  const int64_t *fptr = head ? head_ptr : tail_ptr;
  const int32_t *fidx = head ? head_idx : tail_idx;
  // the block's facts: true score and list bounds, fetched once, straight-line (clamped positions)
  float t[kFB];
  int64_t lo[kFB], hi[kFB];
#pragma unroll
  for (int i = 0; i < kFB; ++i) {
    const int64_t f = f0 + (i < nfb ? i : nfb - 1);
    t[i] = truth[f];
    lo[i] = fptr ? fptr[f] : 0;
    hi[i] = fptr ? fptr[f + 1] : 0;
  }
  if (threadIdx.x < kFB * 4) s_cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;   // (lp_score_tiles opens with a barrier)
  const int lane = threadIdx.x & 63;
  float acc[CT][kFB];
  for (int64_t c0 = 0; c0 < N; c0 += (int64_t)kTB * CT) {
    const int64_t c = c0 + threadIdx.x;
    lp_score_tiles<CT>(Et, N, H, E, ldE, Rel, ldR, head, c, nfb,
                       [&](int fi, int64_t &anchor, int64_t &rel) {
                         const int64_t f = f0 + fi;
                         anchor = tr[3 * f + (head ? 2 : 0)];
                         rel = tr[3 * f + 1];
                       },
                       s_a, s_b, acc);
#pragma unroll
    for (int i = 0; i < kFB; ++i) {
      int ngt = 0, neq = 0, nmgt = 0, nmeq = 0;   // (the wave's counts over its CT candidates per lane)
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int64_t cj = c + (int64_t)j * kTB;
        bool gt = false, eq = false, masked = false;
        if (i < nfb && cj < N) {
          const float sc = (f0 + i) < N ? acc[j][i] : 0.f;
          gt = sc > t[i];
          eq = sc == t[i];
          // (a candidate below the true score counts nowhere: its list is not searched)
          if (fptr && (gt || eq)) masked = in_sorted(fidx, lo[i], hi[i], (int32_t)cj);
        }
        ngt += __popcll(__ballot(gt));
        neq += __popcll(__ballot(eq));
        if (fptr) {
          nmgt += __popcll(__ballot(gt && masked));
          nmeq += __popcll(__ballot(eq && masked));
        }
      }
      if (lane == 0) {
        if (ngt) atomicAdd(&s_cnt[i][0], ngt);
        if (neq) atomicAdd(&s_cnt[i][1], neq);
        if (nmgt) atomicAdd(&s_cnt[i][2], nmgt);
        if (nmeq) atomicAdd(&s_cnt[i][3], nmeq);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < nfb) {
    const int i = threadIdx.x;
    const int64_t at = (head ? nf : 0) + f0 + i;
    const int64_t gt = s_cnt[i][0], eq = s_cnt[i][1];
    raw[at] = lp_rank_of(gt, eq);
    if (fptr) flt[at] = lp_rank_of(gt - s_cnt[i][2], eq - s_cnt[i][3]);
  }
}

// block 0: the raw ranks -> slot[0:4]; block 1: the filtered ranks -> slot[4:8], or -1 four times without lists.  One
// wave each, in k_rank_metrics' order for one part: a lane adds the reciprocals of its ranks (i = lane, lane + 64, ...
// over the 2 nf ranks) in float64 and counts its hits as integers, the lanes are added over the same shuffle tree,
// lane 0 divides by 2 nf and rounds once (that kernel's sums over waves and parts add zeros and divide by one here).
__global__ __launch_bounds__(64) void k_batch_metrics(const int64_t *__restrict__ raw, const int64_t *__restrict__ flt,
                                                      int64_t nf, float *__restrict__ slot) {
  const int lane = threadIdx.x;
  float *out4 = slot + 4 * blockIdx.x;
  const int64_t *ranks = blockIdx.x == 0 ? raw : flt;
  if (ranks == nullptr) {
    if (lane < 4) out4[lane] = -1.f;
    return;
  }
  double rr = 0.0;
  int64_t h1 = 0, h3 = 0, h10 = 0;
  for (int64_t i = lane; i < 2 * nf; i += 64) {
    const int64_t r = ranks[i];
    rr += 1.0 / (double)r;
    h1 += r <= 1 ? 1 : 0;
    h3 += r <= 3 ? 1 : 0;
    h10 += r <= 10 ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    rr += __shfl_down(rr, off, 64);
    h1 += __shfl_down(h1, off, 64);
    h3 += __shfl_down(h3, off, 64);
    h10 += __shfl_down(h10, off, 64);
  }
  if (lane != 0) return;
  const double d = 2.0 * (double)nf;
  out4[0] = (float)(rr / d);
  out4[1] = (float)((double)h1 / d);
  out4[2] = (float)((double)h3 / d);
  out4[3] = (float)((double)h10 / d);
}

// np.mean of the reference's per-batch lists (:331, :416-419): a sequential float64 sum in slot order, one rounding
__global__ void k_lp_batch_means(const float *__restrict__ loss_slots, int64_t n_loss,
                                 const float *__restrict__ train_slots, int64_t n_train,
                                 const float *__restrict__ valid_slots, int64_t n_valid, float *__restrict__ row17,
                                 float *__restrict__ score_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (n_loss > 0) {
    double t = 0.0;
    for (int64_t b = 0; b < n_loss; ++b) t += (double)loss_slots[b];
    row17[0] = (float)(t / (double)n_loss);
  }
  // (a slot's eight values are read together; every column is still added in slot order)
  if (n_train > 0) {
    double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = 0; b < n_train; ++b)
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] += (double)train_slots[8 * b + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) row17[1 + k] = (float)(t[k] / (double)n_train);
  }
  if (n_valid > 0) {
    double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t b = 0; b < n_valid; ++b)
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] += (double)valid_slots[8 * b + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      t[k] /= (double)n_valid;
      row17[9 + k] = (float)t[k];
    }
    if (score_out) *score_out = (float)(1.0 - t[0]);
  }
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int64_t mrgcn_distmult_batch_eval_workspace(int64_t num_nodes, int32_t H, int64_t num_facts) {
  if (num_nodes <= 0 || H <= 0 || num_facts <= 0) return -1;
  if (num_nodes > INT32_MAX || (num_facts + kFB - 1) / kFB > INT32_MAX) return -1;
  // raw ranks [2 nf] int64 | filtered ranks [2 nf] int64 | Et [H, N] floats | truth [nf] floats
  return (int64_t)sizeof(int64_t) * 4 * num_facts + (int64_t)sizeof(float) * ((int64_t)H * num_nodes + num_facts);
}

int mrgcn_distmult_batch_eval(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                              const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                              void *workspace, int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt,
                              float *slot, void *stream) {
  MRGCN_REQUIRE(E && Rel && triples && workspace && slot, "distmult_batch_eval: NULL");
  MRGCN_REQUIRE(H > 0 && num_nodes > 0 && num_facts >= 1 && ldE >= H && ldR >= H,
                "distmult_batch_eval: sizes (num_facts >= 1, ld >= H)");
  MRGCN_REQUIRE((tail_ptr == nullptr) == (head_ptr == nullptr) && (tail_ptr == nullptr) == (tail_idx == nullptr) &&
                    (head_ptr == nullptr) == (head_idx == nullptr),
                "distmult_batch_eval: give all four filter arrays or none");
  const int64_t need = mrgcn_distmult_batch_eval_workspace(num_nodes, H, num_facts);
  MRGCN_REQUIRE(need >= 0 && workspace_bytes >= need, "distmult_batch_eval: workspace too small");
  MRGCN_REQUIRE(((uintptr_t)workspace & 7) == 0, "distmult_batch_eval: workspace on an 8-byte base");
  hipStream_t st = (hipStream_t)stream;
  const bool filtered = tail_ptr != nullptr;
  int64_t *raw = (int64_t *)workspace;
  int64_t *flt = raw + 2 * num_facts;
  float *Et = (float *)(flt + 2 * num_facts);
  float *truth = Et + (int64_t)H * num_nodes;
  if (ranks_raw) raw = ranks_raw;
  if (ranks_flt) flt = ranks_flt;
  const int64_t tiles_c = (num_nodes + 31) / 32, ttiles = tiles_c * ((H + 31) / 32);
  const int64_t tblocks = (num_facts + kTruthFacts - 1) / kTruthFacts;
  MRGCN_REQUIRE(ttiles + tblocks <= INT32_MAX, "distmult_batch_eval: table too large for one grid");
  k_batch_prep<<<dim3((unsigned)(ttiles + tblocks)), dim3(256), 0, st>>>(E, ldE, num_nodes, H, Rel, ldR, triples,
                                                                         num_facts, tiles_c, ttiles, Et, truth);
  MRGCN_HIP_TRY(hipGetLastError());
  dim3 rg((unsigned)((num_facts + kFB - 1) / kFB), 2);
  const int64_t ctiles = (num_nodes + kTB - 1) / kTB;
#define MRGCN_BATCH_RANKS(CT)                                                                                        \
  k_batch_ranks<CT><<<rg, dim3(kTB), 0, st>>>(Et, num_nodes, H, E, ldE, Rel, ldR, triples, num_facts, truth, tail_ptr, \
                                              tail_idx, head_ptr, head_idx, raw, flt)
  if (ctiles <= 1) MRGCN_BATCH_RANKS(1);
  else if (ctiles == 2) MRGCN_BATCH_RANKS(2);
  else if (ctiles == 3) MRGCN_BATCH_RANKS(3);
  else MRGCN_BATCH_RANKS(4);
#undef MRGCN_BATCH_RANKS
  MRGCN_HIP_TRY(hipGetLastError());
  k_batch_metrics<<<dim3(2), dim3(64), 0, st>>>(raw, filtered ? flt : nullptr, num_facts, slot);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_lp_batch_means_f32(const float *loss_slots, int64_t n_loss, const float *train_slots, int64_t n_train,
                             const float *valid_slots, int64_t n_valid, float *row17, float *score_out, void *stream) {
  MRGCN_REQUIRE(row17, "lp_batch_means: NULL");
  MRGCN_REQUIRE(n_loss >= 0 && n_train >= 0 && n_valid >= 0, "lp_batch_means: counts");
  MRGCN_REQUIRE((n_loss == 0 || loss_slots) && (n_train == 0 || train_slots) && (n_valid == 0 || valid_slots),
                "lp_batch_means: a count without its slots");
  k_lp_batch_means<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(loss_slots, n_loss, train_slots, n_train,
                                                                 valid_slots, n_valid, row17, score_out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
