// Link-prediction evaluation inside a replayed epoch (mrgcn_amd.tasks.link_prediction: rank_both, rank_metrics,
// evaluate_facts, fit): what the reference's test_model (tasks/link_prediction.py:375-422) and the early-stop record of
// its train_model (:336-364) do per evaluating epoch, stream ordered, allocation free and without a host read.
//   ranks    raw AND filtered ranks of every fact from ONE pass over the candidate scores (test_model scores twice);
//            the scores are lp_score_tile's, so both equal mrgcn_distmult_ranks' bit for bit
//   metrics  MRR and hits@{1,3,10} of a rank vector as the mean over parts of the part means (:403-419), float64 in a
//            fixed order
//   record   the early-stop record with a metrics row of any width
#include "common.hpp"
#include "early_stop.hpp"
#include "lp_score.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = kLpTB;
constexpr int kFB = kLpFB;
constexpr int kHT = kLpHT;
constexpr int64_t kMaxSliceFacts = (int64_t)65535 * kFB;   // grid.y of one launch
constexpr int64_t kSliceFacts = (int64_t)32768 * kFB;      // the default slice: 262 144 facts per launch

// counts[8 f + 4 dir + w], w: 0 greater, 1 ties (all live candidates), 2 masked and greater, 3 masked and tie.
// The filtered counts are (0) - (2) and (1) - (3): the lists are short, so (2) and (3) are nearly always zero and their
// LDS / global atomics are skipped, where four independent counters would pay all four for every fact.

// truth[f] as k_true_scores writes it.  The reference leaves the facts at positions >= num_nodes OF ITS CALL unscored
// (link_prediction.py:611-617); a call here stands for one call per part, so the position is the one inside the part.
// SC == kLpComplEx: the two sides round differently (lp_score.hpp: lp_stage), so the fact's own score is kept PER SIDE,
// truth[f] by the tail side's operations and truth[nf + f] by the head side's — the fact's own answer then ties with
// itself exactly, as lp_rank_of assumes.
template <int SC>
__global__ void k_truth_both(const float *__restrict__ E, int64_t ldE, const float *__restrict__ Rel, int64_t ldR,
                             int H, const int64_t *__restrict__ tr, int64_t nf, int64_t N,
                             const int64_t *__restrict__ part_ptr, int64_t nparts, float *__restrict__ truth,
                             int32_t *__restrict__ scored, int32_t *__restrict__ counts) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) counts[8 * f + k] = 0;
  int64_t pos = f;
  if (part_ptr) {   // the last part that starts at or before f
    int64_t lo = 0, hi = nparts - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (part_ptr[mid] <= f) lo = mid; else hi = mid - 1;
    }
    pos = f - part_ptr[lo];
  }
  float acc = 0.f;
  if constexpr (SC == kLpComplEx) {
    float acc_h = 0.f;
    if (pos < N) {
      const int64_t si = tr[3 * f], pi = tr[3 * f + 1], oi = tr[3 * f + 2];
      const float *s = E + si * ldE, *o = E + oi * ldE;
      for (int h = 0; h < H; ++h) {
        float qt, qh, unused;
        lp_stage<SC>(E, ldE, Rel, ldR, H, false, si, pi, h, qt, unused);
        lp_stage<SC>(E, ldE, Rel, ldR, H, true, oi, pi, h, qh, unused);
        const float pt = qt * o[h];
        const float ph = qh * s[h];
        acc = acc + pt;
        acc_h = acc_h + ph;
      }
    }
    truth[nf + f] = acc_h;
  } else if (pos < N) {
    const float *s = E + tr[3 * f] * ldE, *p = Rel + tr[3 * f + 1] * ldR, *o = E + tr[3 * f + 2] * ldE;
    for (int h = 0; h < H; ++h) {
      const float sp = s[h] * p[h];
      const float spo = sp * o[h];
      acc = acc + spo;
    }
  }
  truth[f] = acc;
  scored[f] = pos < N ? 1 : 0;
}

// grid (candidate tiles, fact tiles of this slice, 2 directions): k_rank_counts' grid, facts from f_begin on.
template <int SC>
__global__ __launch_bounds__(kTB) void k_rank_counts_both(
    const float *__restrict__ Et, int64_t N, int H, const float *__restrict__ E, int64_t ldE,
    const float *__restrict__ Rel, int64_t ldR, const int64_t *__restrict__ tr, int64_t nf, int64_t f_begin,
    const float *__restrict__ truth, const int32_t *__restrict__ scored, const int64_t *__restrict__ tail_ptr,
    const int32_t *__restrict__ tail_idx, const int64_t *__restrict__ head_ptr,
    const int32_t *__restrict__ head_idx, int32_t *__restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ float s_a[kFB][kHT];
  __shared__ float s_b[kFB][kHT];
  __shared__ int s_cnt[kFB][4];
  const bool head = blockIdx.z == 1;
  const int64_t c = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t f0 = f_begin + (int64_t)blockIdx.y * kFB;
  const int nfb = (int)((nf - f0) < kFB ? (nf - f0) : kFB);
  const bool live = c < N;
  float acc[kFB];
  if (threadIdx.x < kFB * 4) s_cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;
  lp_score_tile<SC>(Et, N, H, E, ldE, Rel, ldR, head, c, live, nfb,
                [&](int fi, int64_t &anchor, int64_t &rel) {
                  const int64_t f = f0 + fi;
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
      const int64_t f = f0 + i;
      const float sc = scored[f] ? acc[i] : 0.f;
      const float t = truth[(SC == kLpComplEx && head ? nf : 0) + f];
      gt = sc > t;
      eq = sc == t;
      // (a candidate below the true score counts nowhere: its list is not searched)
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
    if (v) atomicAdd(&counts[8 * (f0 + i) + (head ? 4 : 0) + w], v);
  }
}

__global__ void k_rank_final_both(const int32_t *__restrict__ counts, int64_t nf, int64_t *__restrict__ raw,
                                  int64_t *__restrict__ flt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * nf) return;
  const bool head = i >= nf;
  const int32_t *cn = counts + 8 * (head ? i - nf : i) + (head ? 4 : 0);
  const int64_t gt = cn[0], eq = cn[1];
  raw[i] = lp_rank_of(gt, eq);
  if (flt) flt[i] = lp_rank_of(gt - cn[2], eq - cn[3]);
}

// ---- rank metrics ----------------------------------------------------------------------------------------------------
// One block; a wave takes the parts wave, wave + 16, ...  A lane adds the reciprocals of its ranks of the part (tail
// ranks, then head ranks, rising) in float64 and counts its hits as integers; the lanes are added over a fixed shuffle
// tree; lane 0 divides by the part's 2 n ranks and adds the part's means to the wave's in part order; thread 0 adds the
// waves in wave order, divides by the number of parts and rounds once to float32.  No atomics: equal inputs, equal bits.
constexpr int kMetTB = 1024;
constexpr int kMetWaves = kMetTB / 64;

__global__ __launch_bounds__(kMetTB) void k_rank_metrics(const int64_t *__restrict__ ranks, int64_t nf,
                                                         const int64_t *__restrict__ part_ptr, int64_t nparts,
                                                         float *__restrict__ out4, float *__restrict__ score_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // (meaningful in lane 0)
  for (int64_t p = wave; p < nparts; p += kMetWaves) {
    int64_t p0 = part_ptr ? part_ptr[p] : 0, p1 = part_ptr ? part_ptr[p + 1] : nf;
    // (the caller guarantees 0 = ptr[0] <= ... <= ptr[nparts] = nf; whatever it passes, no read leaves `ranks`)
    p0 = p0 < 0 ? 0 : (p0 > nf ? nf : p0);
    p1 = p1 < p0 ? p0 : (p1 > nf ? nf : p1);
    const int64_t n = p1 - p0;
    double rr = 0.0;
    int64_t h1 = 0, h3 = 0, h10 = 0;
    for (int64_t i = lane; i < 2 * n; i += 64) {
      const int64_t r = ranks[i < n ? p0 + i : nf + p0 + (i - n)];
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
    if (n > 0) {
      const double d = 2.0 * (double)n;
      acc[0] += rr / d;
      acc[1] += (double)h1 / d;
      acc[2] += (double)h3 / d;
      acc[3] += (double)h10 / d;
    }
  }
  __shared__ double s_acc[kMetWaves][4];
  if (lane == 0)
    for (int k = 0; k < 4; ++k) s_acc[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < kMetWaves; ++w)
    for (int k = 0; k < 4; ++k) t[k] += s_acc[w][k];
  for (int k = 0; k < 4; ++k) {
    t[k] /= (double)nparts;
    out4[k] = (float)t[k];
  }
  if (score_out) *score_out = (float)(1.0 - t[0]);
}

// ---- the early-stop record with a row of `width` floats -------------------------------------------------------------
__global__ void k_early_stop_record_row(mrgcn_early_stop_state *__restrict__ st, const float *__restrict__ score,
                                        double tolerance, int patience_default, const float *__restrict__ row,
                                        int width, float *__restrict__ ring, int64_t rows) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (!early_stop_open(st)) return;
  float *dst = ring + (st->records % rows) * width;
  for (int k = 0; k < width; ++k) dst[k] = row[k];
  early_stop_book(st, score, tolerance, patience_default);
}

// Et [H, N] floats | truth [sides nf] floats | scored [nf] int32 | counts [8 nf] int32
inline int64_t ranks_both_bytes(int64_t num_nodes, int32_t H, int64_t num_facts, int sides) {
  if (num_nodes < 0 || H <= 0 || num_facts < 0) return -1;
  return (int64_t)sizeof(float) * ((int64_t)H * num_nodes + sides * num_facts) +
         (int64_t)sizeof(int32_t) * 9 * num_facts;
}

template <int SC>
int ranks_both_run(const char *who_, const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR,
                   int32_t H, const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                   const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx, const int64_t *part_ptr,
                   int64_t num_parts, int64_t slice_facts, void *workspace, int64_t workspace_bytes,
                   int64_t *ranks_raw, int64_t *ranks_flt, void *stream) {
  const std::string who(who_);
  constexpr int kSides = SC == kLpComplEx ? 2 : 1;
  MRGCN_REQUIRE(E && Rel && triples && ranks_raw && workspace && H > 0 && num_nodes > 0 && num_facts >= 0,
                who + ": bad argument");
  MRGCN_REQUIRE((tail_ptr == nullptr) == (head_ptr == nullptr) && (tail_ptr == nullptr) == (tail_idx == nullptr) &&
                    (head_ptr == nullptr) == (head_idx == nullptr),
                who + ": give all four filter arrays or none");
  MRGCN_REQUIRE(tail_ptr == nullptr || ranks_flt != nullptr, who + ": filter lists without ranks_flt");
  MRGCN_REQUIRE(part_ptr == nullptr || num_parts > 0, who + ": part_ptr without parts");
  MRGCN_REQUIRE(slice_facts >= 0 && slice_facts <= kMaxSliceFacts, who + ": slice_facts");
  MRGCN_REQUIRE(workspace_bytes >= ranks_both_bytes(num_nodes, H, num_facts, kSides), who + ": workspace too small");
  if (num_facts == 0) return MRGCN_OK;
  hipStream_t st = (hipStream_t)stream;
  float *Et = (float *)workspace;
  float *truth = Et + (int64_t)H * num_nodes;
  int32_t *scored = (int32_t *)(truth + kSides * num_facts);
  int32_t *counts = scored + num_facts;
  MRGCN_HIP_TRY(lp_transpose(E, ldE, num_nodes, H, Et, st));
  k_truth_both<SC><<<(unsigned)((num_facts + 127) / 128), 128, 0, st>>>(E, ldE, Rel, ldR, H, triples, num_facts,
                                                                         num_nodes, part_ptr, num_parts, truth, scored,
                                                                         counts);
  MRGCN_HIP_TRY(hipGetLastError());
  int64_t slice = slice_facts > 0 ? slice_facts : kSliceFacts;
  slice = (slice + kFB - 1) / kFB * kFB;   // whole fact tiles
  const bool filtered = tail_ptr != nullptr;
  for (int64_t f0 = 0; f0 < num_facts; f0 += slice) {
    const int64_t m = (num_facts - f0) < slice ? (num_facts - f0) : slice;
    dim3 rg((unsigned)((num_nodes + kTB - 1) / kTB), (unsigned)((m + kFB - 1) / kFB), 2);
    k_rank_counts_both<SC><<<rg, kTB, 0, st>>>(Et, num_nodes, H, E, ldE, Rel, ldR, triples, num_facts, f0, truth,
                                               scored, tail_ptr, tail_idx, head_ptr, head_idx, counts);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  k_rank_final_both<<<(unsigned)((2 * num_facts + 255) / 256), 256, 0, st>>>(counts, num_facts, ranks_raw,
                                                                            filtered ? ranks_flt : nullptr);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" {

int64_t mrgcn_distmult_ranks_both_slice(void) { return kSliceFacts; }

int64_t mrgcn_distmult_ranks_both_workspace(int64_t num_nodes, int32_t H, int64_t num_facts) {
  return ranks_both_bytes(num_nodes, H, num_facts, 1);
}

int mrgcn_distmult_ranks_both(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                              const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                              const int64_t *part_ptr, int64_t num_parts, int64_t slice_facts, void *workspace,
                              int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt, void *stream) {
  return ranks_both_run<kLpDistMult>("distmult_ranks_both", E, ldE, num_nodes, Rel, ldR, H, triples, num_facts,
                                     tail_ptr, tail_idx, head_ptr, head_idx, part_ptr, num_parts, slice_facts,
                                     workspace, workspace_bytes, ranks_raw, ranks_flt, stream);
}

// The ComplEx twins (Trouillon et al. 2016): the same contract word for word; the scores are lp_stage<kLpComplEx>'s and
// the fact's own score is kept per side (truth [2 nf]).
int64_t mrgcn_complex_ranks_both_workspace(int64_t num_nodes, int32_t H, int64_t num_facts) {
  return ranks_both_bytes(num_nodes, H, num_facts, 2);
}

int mrgcn_complex_ranks_both(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                             const int64_t *triples, int64_t num_facts, const int64_t *tail_ptr,
                             const int32_t *tail_idx, const int64_t *head_ptr, const int32_t *head_idx,
                             const int64_t *part_ptr, int64_t num_parts, int64_t slice_facts, void *workspace,
                             int64_t workspace_bytes, int64_t *ranks_raw, int64_t *ranks_flt, void *stream) {
  MRGCN_REQUIRE(H > 0 && H % 2 == 0, "complex_ranks_both: H must be even (H / 2 complex numbers per row)");
  return ranks_both_run<kLpComplEx>("complex_ranks_both", E, ldE, num_nodes, Rel, ldR, H, triples, num_facts,
                                    tail_ptr, tail_idx, head_ptr, head_idx, part_ptr, num_parts, slice_facts,
                                    workspace, workspace_bytes, ranks_raw, ranks_flt, stream);
}

int mrgcn_rank_metrics(const int64_t *ranks, int64_t num_facts, const int64_t *part_ptr, int64_t num_parts, float *out4,
                       float *score_out, void *stream) {
  MRGCN_REQUIRE(ranks && out4 && num_facts > 0 && num_parts > 0, "rank_metrics: bad argument");
  MRGCN_REQUIRE(part_ptr != nullptr || num_parts == 1, "rank_metrics: more than one part needs part_ptr");
  k_rank_metrics<<<dim3(1), dim3(kMetTB), 0, (hipStream_t)stream>>>(ranks, num_facts, part_ptr, num_parts, out4,
                                                                   score_out);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_early_stop_record_row(mrgcn_early_stop_state *state, const float *score, double tolerance,
                                int32_t patience_default, const float *row, int32_t width, float *ring, int64_t rows,
                                void *stream) {
  MRGCN_REQUIRE(state && score && row && ring, "NULL");
  MRGCN_REQUIRE(width > 0 && rows > 0, "early_stop_record_row: width / rows");
  k_early_stop_record_row<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(state, score, tolerance, patience_default, row,
                                                                        width, ring, rows);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
