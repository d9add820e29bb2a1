// Validation and early stopping inside the replayed epoch (mrgcn_amd.train: evaluate, DeviceEarlyStop,
// GraphedTrainEvalStep): the evaluation loss and accuracy of a label set, the bookkeeping of the reference's
// tasks/utils.py::EarlyStop on a small device struct, and the copy of the best parameters and optimizer state that a
// device flag switches on.  Everything is stream ordered and allocation free, so a hipGraph replays it.
#include <cmath>

#include "common.hpp"
#include "early_stop.hpp"

namespace mrgcn {

// ---- evaluation loss and accuracy ------------------------------------------------------------------------------------
// One thread per labelled row; a thread adds its rows in rising order, a block adds its threads over a fixed tree
// (lanes, then waves in order), blocks are added in block order by k_xent_eval_final: the same bits on every call.
constexpr int kEvalTB = 256;
constexpr int kEvalSingle = 4096;      // rows one block takes alone (16 per thread)
constexpr int kEvalMaxBlocks = 256;

struct EvalPart {
  double loss;
  int64_t correct;
};

__device__ __forceinline__ EvalPart eval_block_part(const float *__restrict__ logits, int64_t ld, int C,
                                                    const int64_t *__restrict__ idx,
                                                    const int64_t *__restrict__ target, int64_t n,
                                                    int64_t *__restrict__ labels) {
  double my = 0.0;
  int64_t ok = 0;
  const int64_t stride = (int64_t)gridDim.x * kEvalTB;
  for (int64_t i = (int64_t)blockIdx.x * kEvalTB + threadIdx.x; i < n; i += stride) {
    const float *z = logits + idx[i] * ld;
    const int64_t t = target[i];
    float mx = z[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {  // strict >: of equal values the lowest class stays (Tensor.max(dim=1))
      const float v = z[c];
      if (v > mx) {
        mx = v;
        am = c;
      }
    }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
    const float lse = logf(se) + mx;
    const float zt = (t >= 0 && t < C) ? z[t] : NAN;  // (a target outside the classes poisons the loss, reads nothing)
    my += (double)(lse - zt);
    ok += (int64_t)am == t ? 1 : 0;
    if (labels) labels[i] = am;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    my += __shfl_down(my, off, 64);
    ok += __shfl_down(ok, off, 64);
  }
  __shared__ double s_loss[kEvalTB / 64];
  __shared__ int64_t s_ok[kEvalTB / 64];
  if ((threadIdx.x & 63) == 0) {
    s_loss[threadIdx.x >> 6] = my;
    s_ok[threadIdx.x >> 6] = ok;
  }
  __syncthreads();
  EvalPart p{0.0, 0};
  if (threadIdx.x == 0)
    for (int w = 0; w < kEvalTB / 64; ++w) {
      p.loss += s_loss[w];
      p.correct += s_ok[w];
    }
  return p;  // (meaningful in thread 0)
}

__global__ __launch_bounds__(kEvalTB) void k_xent_eval(const float *__restrict__ logits, int64_t ld, int C,
                                                       const int64_t *__restrict__ idx,
                                                       const int64_t *__restrict__ target, int64_t n,
                                                       float *__restrict__ loss, int64_t *__restrict__ correct,
                                                       int64_t *__restrict__ labels, EvalPart *__restrict__ parts) {
  const EvalPart p = eval_block_part(logits, ld, C, idx, target, n, labels);
  if (threadIdx.x != 0) return;
  if (parts) {
    parts[blockIdx.x] = p;
  } else {
    *loss = (float)(p.loss / (double)n);
    *correct = p.correct;
  }
}

__global__ void k_xent_eval_final(const EvalPart *__restrict__ parts, int nparts, int64_t n, float *__restrict__ loss,
                                  int64_t *__restrict__ correct) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double t = 0.0;
  int64_t ok = 0;
  for (int b = 0; b < nparts; ++b) {
    t += parts[b].loss;
    ok += parts[b].correct;
  }
  *loss = (float)(t / (double)n);
  *correct = ok;
}

// ---- tasks/utils.py:64-81 on the device -----------------------------------------------------------------------------
struct MetricsRow {
  const float *src[4];
  float *ring;
  int64_t rows;
};

__global__ void k_early_stop_record(mrgcn_early_stop_state *__restrict__ st, const float *__restrict__ score,
                                    double tolerance, int patience_default, MetricsRow m) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (!early_stop_open(st)) return;
  if (m.ring) {
    float *row = m.ring + (st->records % m.rows) * 4;
    for (int k = 0; k < 4; ++k) row[k] = m.src[k] ? *m.src[k] : -1.f;
  }
  early_stop_book(st, score, tolerance, patience_default);
}

// ---- the snapshot: table-driven copy behind a device flag ------------------------------------------------------------
// One-shot grid: block b copies kSnapBlockBytes of the entry whose block range holds b (entries with no bytes have no
// blocks).  16-byte stores at 16-byte aligned addresses; what lies in front of the first and behind the last such
// address inside the block's piece goes byte by byte.  Loads are 16-byte loads when source and destination sit at the
// same offset inside 16 bytes, and assembled from the alignment the source has otherwise.
constexpr int kSnapTB = 256;
constexpr int kSnapPerThread = 4;
constexpr int64_t kSnapBlockBytes = (int64_t)kSnapTB * kSnapPerThread * 16;

struct __attribute__((packed, aligned(1))) Bytes16 {
  unsigned char b[16];
};

__global__ __launch_bounds__(kSnapTB) void k_snapshot_if(const int32_t *__restrict__ flag,
                                                         const mrgcn_copy_entry *__restrict__ table, int n_entries,
                                                         int restore) {
  if (flag && *flag == 0) return;
  // the last entry whose first block is <= this block (first_block rises; empty entries share their successor's)
  int lo = 0, hi = n_entries - 1;
  const int64_t b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const mrgcn_copy_entry e = table[lo];
  const int64_t off = (b - e.first_block) * kSnapBlockBytes;
  if (off < 0 || off >= e.bytes) return;
  const int64_t len = e.bytes - off < kSnapBlockBytes ? e.bytes - off : kSnapBlockBytes;
  const unsigned char *s = (const unsigned char *)(restore ? e.dst : e.src) + off;
  unsigned char *d = (unsigned char *)(restore ? e.src : e.dst) + off;
  int64_t head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15);
  if (head > len) head = len;
  const int64_t nvec = (len - head) >> 4;
  const int64_t tail0 = head + (nvec << 4);
  const int tid = threadIdx.x;
  if (tid < head) d[tid] = s[tid];
  const int tt = tid - 64;  // (the second wave's lanes take the bytes behind the last whole 16)
  if (tt >= 0 && tt < 16 && tail0 + tt < len) d[tail0 + tt] = s[tail0 + tt];
  uint4 *d4 = reinterpret_cast<uint4 *>(d + head);
  if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(s + head);
    uint4 r[kSnapPerThread];
#pragma unroll
    for (int u = 0; u < kSnapPerThread; ++u) {
      const int64_t i = tid + u * kSnapTB;
      if (i < nvec) r[u] = s4[i];
    }
#pragma unroll
    for (int u = 0; u < kSnapPerThread; ++u) {
      const int64_t i = tid + u * kSnapTB;
      if (i < nvec) d4[i] = r[u];
    }
  } else {
    const Bytes16 *sb = reinterpret_cast<const Bytes16 *>(s + head);
#pragma unroll
    for (int u = 0; u < kSnapPerThread; ++u) {
      const int64_t i = tid + u * kSnapTB;
      if (i < nvec) {
        const Bytes16 v = sb[i];
        uint4 w;
        __builtin_memcpy(&w, &v, 16);
        d4[i] = w;
      }
    }
  }
}

}  // namespace mrgcn

extern "C" {

int64_t mrgcn_xent_eval_workspace(void) { return (int64_t)mrgcn::kEvalMaxBlocks * (int64_t)sizeof(mrgcn::EvalPart); }
int64_t mrgcn_xent_eval_single_block_rows(void) { return mrgcn::kEvalSingle; }

int mrgcn_xent_eval_rows_f32(const float *logits, int64_t ld, int32_t C, const int64_t *idx, const int64_t *target,
                             int64_t n, float *loss_out, int64_t *correct_out, int64_t *labels_out, void *workspace,
                             void *stream) {
  MRGCN_REQUIRE(logits && idx && target && loss_out && correct_out, "NULL");
  MRGCN_REQUIRE(C > 0 && ld >= C && n > 0, "C / ld / n");
  hipStream_t s = (hipStream_t)stream;
  if (n <= mrgcn::kEvalSingle) {
    mrgcn::k_xent_eval<<<dim3(1), dim3(mrgcn::kEvalTB), 0, s>>>(logits, ld, C, idx, target, n, loss_out, correct_out,
                                                                 labels_out, nullptr);
    MRGCN_HIP_TRY(hipGetLastError());
    return MRGCN_OK;
  }
  MRGCN_REQUIRE(workspace, "more rows than one block takes: workspace of mrgcn_xent_eval_workspace() bytes");
  int64_t grid = (n + mrgcn::kEvalTB - 1) / mrgcn::kEvalTB;  // (a function of n only)
  if (grid > mrgcn::kEvalMaxBlocks) grid = mrgcn::kEvalMaxBlocks;
  mrgcn::EvalPart *parts = (mrgcn::EvalPart *)workspace;
  mrgcn::k_xent_eval<<<dim3((unsigned)grid), dim3(mrgcn::kEvalTB), 0, s>>>(logits, ld, C, idx, target, n, loss_out,
                                                                           correct_out, labels_out, parts);
  MRGCN_HIP_TRY(hipGetLastError());
  mrgcn::k_xent_eval_final<<<dim3(1), dim3(64), 0, s>>>(parts, (int)grid, n, loss_out, correct_out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_early_stop_record(mrgcn_early_stop_state *state, const float *score, double tolerance,
                            int32_t patience_default, const mrgcn_metrics_row *metrics_row, void *stream) {
  MRGCN_REQUIRE(state && score, "NULL");
  mrgcn::MetricsRow m{{nullptr, nullptr, nullptr, nullptr}, nullptr, 0};
  if (metrics_row) {
    MRGCN_REQUIRE(metrics_row->ring && metrics_row->rows > 0, "metrics_row: ring / rows");
    for (int k = 0; k < 4; ++k) m.src[k] = metrics_row->values[k];
    m.ring = metrics_row->ring;
    m.rows = metrics_row->rows;
  }
  mrgcn::k_early_stop_record<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(state, score, tolerance, patience_default, m);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int64_t mrgcn_snapshot_block_bytes(void) { return mrgcn::kSnapBlockBytes; }

int mrgcn_snapshot_if(const int32_t *flag, const mrgcn_copy_entry *table, int32_t n_entries, int64_t n_blocks,
                      int32_t restore, void *stream) {
  MRGCN_REQUIRE(table || n_entries == 0, "NULL");
  MRGCN_REQUIRE(n_entries >= 0 && n_blocks >= 0 && n_blocks < ((int64_t)1 << 31), "n_entries / n_blocks");
  if (n_entries == 0 || n_blocks == 0) return MRGCN_OK;
  mrgcn::k_snapshot_if<<<dim3((unsigned)n_blocks), dim3(mrgcn::kSnapTB), 0, (hipStream_t)stream>>>(flag, table, n_entries,
                                                                                                   restore);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
