// Mini-batch node classification on fixed batches (mrgcn_amd.tasks.node_classification: train_batch_step, eval_model,
// test_model, BatchEpoch): what one batch of node_classification.py:158-201 / :229-256 takes from its logits — loss,
// compact gradient rows, correct arg-maxes, labels, the batch's {loss, accuracy} slot — in ONE pass over the labelled
// rows, and the epoch's unweighted means over the batches' slots (:203-204, :253-254).  Stream ordered, allocation
// free, no atomics: a hipGraph replays an epoch of them and equal inputs give equal bits.
#include <cmath>

#include "common.hpp"
#include "xent_row.hpp"

namespace mrgcn {
namespace {

constexpr int kNcTB = 1024;
constexpr int kNcSingle = 4096;      // rows one block takes alone (4 per thread)
constexpr int kNcMaxBlocks = 256;

struct NcPart {
  double loss;
  int64_t correct;
};

// One thread per labelled row.  The row itself — loads, softmax, gradient row, arg-max — is xent_row (xent_row.hpp),
// the one body k_xent_rows (optim.hip) runs too, so the rows of `drows` are its bits; the arg-max rule and the
// poisoned target are k_xent_eval's (early_stop.hip).  A thread adds its rows in rising order in float64, the block
// adds its threads over a fixed tree (lanes, then waves in order).  The part is meaningful in thread 0.
__device__ __forceinline__ NcPart nc_block_part(const float *__restrict__ logits, int64_t ld, int C,
                                                const int64_t *__restrict__ idx, const int64_t *__restrict__ target,
                                                int64_t n, float *__restrict__ drows, int64_t *__restrict__ labels) {
  double my = 0.0;
  int64_t ok = 0;
  const float inv_n = 1.f / (float)n;
  const int64_t stride = (int64_t)gridDim.x * kNcTB;
  const int64_t first = (int64_t)blockIdx.x * kNcTB + threadIdx.x;
  // (the next row's index and target are fetched under this row's work, at a clamped position)
  int64_t row_n = idx[first < n ? first : n - 1], t_n = target[first < n ? first : n - 1];
  for (int64_t i = first; i < n; i += stride) {
    const float *z = logits + row_n * ld;
    const int64_t t = t_n;
    {
      const int64_t nx = i + stride < n ? i + stride : n - 1;
      row_n = idx[nx];
      t_n = target[nx];
    }
    const XentRow r = xent_row(z, C, t, inv_n, drows ? drows + i * C : nullptr);
    const int am = r.am;
    const float lse = r.lse;
    float zt = r.zt;
    const bool t_ok = t >= 0 && t < C;
    if (!t_ok) zt = NAN;  // (a target outside the classes poisons the loss and reads nothing)
    my += (double)(lse - zt);
    ok += (int64_t)am == t ? 1 : 0;
    if (labels) labels[i] = am;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    my += __shfl_down(my, off, 64);
    ok += __shfl_down(ok, off, 64);
  }
  __shared__ double s_loss[kNcTB / 64];
  __shared__ int64_t s_ok[kNcTB / 64];
  if ((threadIdx.x & 63) == 0) {
    s_loss[threadIdx.x >> 6] = my;
    s_ok[threadIdx.x >> 6] = ok;
  }
  __syncthreads();
  NcPart p{0.0, 0};
  if (threadIdx.x == 0)
    for (int w = 0; w < kNcTB / 64; ++w) {
      p.loss += s_loss[w];
      p.correct += s_ok[w];
    }
  return p;
}

__device__ __forceinline__ void nc_write(double sum, int64_t ok, int64_t n, float *__restrict__ loss,
                                         int64_t *__restrict__ correct, float *__restrict__ slot) {
  const float l = (float)(sum / (double)n);
  *loss = l;
  *correct = ok;
  if (slot) {
    slot[0] = l;
    slot[1] = (float)ok / (float)n;
  }
}

__global__ __launch_bounds__(kNcTB) void k_nc_xent(const float *__restrict__ logits, int64_t ld, int C,
                                                   const int64_t *__restrict__ idx, const int64_t *__restrict__ target,
                                                   int64_t n, float *__restrict__ loss, float *__restrict__ drows,
                                                   int64_t *__restrict__ correct, int64_t *__restrict__ labels,
                                                   float *__restrict__ slot, NcPart *__restrict__ parts) {
  const NcPart p = nc_block_part(logits, ld, C, idx, target, n, drows, labels);
  if (threadIdx.x != 0) return;
  if (parts)
    parts[blockIdx.x] = p;
  else
    nc_write(p.loss, p.correct, n, loss, correct, slot);
}

__global__ void k_nc_xent_final(const NcPart *__restrict__ parts, int nparts, int64_t n, float *__restrict__ loss,
                                int64_t *__restrict__ correct, float *__restrict__ slot) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double t = 0.0;
  int64_t ok = 0;
  for (int b = 0; b < nparts; ++b) {
    t += parts[b].loss;
    ok += parts[b].correct;
  }
  nc_write(t, ok, n, loss, correct, slot);
}

// np.mean of the reference's per-batch lists: a sequential float64 sum in slot order, one rounding to float32
__global__ void k_nc_batch_means(const float *__restrict__ train_slots, int64_t n_train,
                                 const float *__restrict__ valid_slots, int64_t n_valid, float *__restrict__ row4) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double tl = 0.0, ta = 0.0;
  for (int64_t b = 0; b < n_train; ++b) {
    tl += (double)train_slots[2 * b];
    ta += (double)train_slots[2 * b + 1];
  }
  row4[0] = (float)(tl / (double)n_train);
  row4[1] = (float)(ta / (double)n_train);
  if (n_valid <= 0) {
    row4[2] = -1.f;
    row4[3] = -1.f;
    return;
  }
  double vl = 0.0, va = 0.0;
  for (int64_t b = 0; b < n_valid; ++b) {
    vl += (double)valid_slots[2 * b];
    va += (double)valid_slots[2 * b + 1];
  }
  row4[2] = (float)(vl / (double)n_valid);
  row4[3] = (float)(va / (double)n_valid);
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int64_t mrgcn_xent_train_eval_workspace(void) { return (int64_t)kNcMaxBlocks * (int64_t)sizeof(NcPart); }
int64_t mrgcn_xent_train_eval_single_block_rows(void) { return kNcSingle; }

int mrgcn_xent_train_eval_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx,
                                   const int64_t *target, int64_t n, float *loss, float *drows, int64_t *correct,
                                   int64_t *labels, float *slot, void *workspace, void *stream) {
  MRGCN_REQUIRE(logits && idx && target && loss && correct, "NULL");
  MRGCN_REQUIRE(C > 0 && ld >= C && n > 0, "C / ld / n");
  hipStream_t s = (hipStream_t)stream;
  if (n <= kNcSingle) {
    k_nc_xent<<<dim3(1), dim3(kNcTB), 0, s>>>(logits, ld, C, idx, target, n, loss, drows, correct, labels, slot,
                                              nullptr);
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  MRGCN_REQUIRE(workspace, "more rows than one block takes: workspace of mrgcn_xent_train_eval_workspace() bytes");
  int64_t grid = (n + kNcTB - 1) / kNcTB;  // (a function of n only)
  if (grid > kNcMaxBlocks) grid = kNcMaxBlocks;
  NcPart *parts = (NcPart *)workspace;
  k_nc_xent<<<dim3((unsigned)grid), dim3(kNcTB), 0, s>>>(logits, ld, C, idx, target, n, loss, drows, correct, labels,
                                                         slot, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  k_nc_xent_final<<<dim3(1), dim3(64), 0, s>>>(parts, (int)grid, n, loss, correct, slot);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_batch_means_f32(const float *train_slots, int64_t n_train, const float *valid_slots, int64_t n_valid,
                          float *row4, void *stream) {
  MRGCN_REQUIRE(train_slots && row4, "NULL");
  MRGCN_REQUIRE(n_train > 0 && n_valid >= 0, "batch_means: n_train / n_valid");
  MRGCN_REQUIRE(n_valid == 0 || valid_slots, "batch_means: validation slots");
  k_nc_batch_means<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(train_slots, n_train, valid_slots, n_valid, row4);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
