// Top-k candidate completion behind the DistMult decoder: for every query (s, p, ?) or (?, p, o) the k best nodes.
// The reference answers this with the [facts, nodes] score matrix of compute_ranks_fast
// (mrgcn/tasks/link_prediction.py:593-643, scores :645-665) and a sort over it; here the matrix is never written:
//   pass 1  k_topk_tiles   a block scores 256 candidates against 8 queries with the rank kernel's own scoring body
//                          (lp_score.hpp: the same bits), packs (score, node) into 64-bit keys whose unsigned order IS
//                          the result order, sorts each query's 256 keys in LDS (bitonic network, 36 stages) and
//                          leaves the first k as the tile's list,
//   pass 2  k_topk_merge   one block per query folds the tile lists, in tile order, into a sorted buffer of
//                          K = 2^ceil(log2 k) keys (a 2K bitonic merge per list) and decodes the first k.
// Keys are unique per candidate (the node id is part of the key), so the result is a pure function of the inputs: no
// atomics, nothing depends on which block arrives first.
#include <algorithm>

#include "common.hpp"
#include "lp_score.hpp"

namespace mrgcn {
namespace {

constexpr int kTopkMax = 256;  // k at most: a tile's list is cut from ONE sorted tile of kLpTB candidates
static_assert(kTopkMax <= kLpTB, "a tile list cannot be longer than the tile");

// Unsigned order of the key = result order: score descending (-0 counts as +0), then node id ascending.  0 = no
// candidate (excluded, or past N): below every key of a finite score.
__device__ __forceinline__ uint64_t topk_key(float score, int64_t c) {
  uint32_t u = __float_as_uint(score);
  if (u == 0x80000000u) u = 0u;
  const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)o << 32) | (uint32_t)~(uint32_t)c;
}

// Bitonic sort of each query's kLpTB keys, descending: kLpTB / 2 comparators per query and stage, two queries at a time.
// Every thread of the block calls it; the keys are sorted (and visible) on return.
__device__ __forceinline__ void topk_sort_tile(uint64_t (*s_key)[kLpTB], int nfb) {
  const int t = threadIdx.x & (kLpTB / 2 - 1);
  for (int size = 2; size <= kLpTB; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
      const bool desc = (lo & size) == 0;
      for (int i = threadIdx.x / (kLpTB / 2); i < nfb; i += 2) {
        const uint64_t a = s_key[i][lo], b = s_key[i][hi];
        if ((a < b) == desc) {
          s_key[i][lo] = b;
          s_key[i][hi] = a;
        }
      }
    }
  }
  __syncthreads();
}

// grid (candidate tiles, query tiles).  part[(q * ntiles + tile) * k + j] = key j of the tile's sorted list
template <int SC>
__global__ __launch_bounds__(kLpTB) void k_topk_tiles(
    const float *__restrict__ Et, int64_t N, int H, const float *__restrict__ E, int64_t ldE,
    const float *__restrict__ Rel, int64_t ldR, const int64_t *__restrict__ queries, int64_t nq, int head_,
    const int64_t *__restrict__ excl_ptr, const int32_t *__restrict__ excl_idx, int k, int64_t ntiles,
    uint64_t *__restrict__ part) {
  __shared__ float s_a[kLpFB][kLpHT];
  __shared__ float s_b[kLpFB][kLpHT];
  __shared__ uint64_t s_key[kLpFB][kLpTB];
  const bool head = head_ != 0;
  const int64_t c = (int64_t)blockIdx.x * kLpTB + threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * kLpFB;
  const int nfb = (int)((nq - q0) < kLpFB ? (nq - q0) : kLpFB);
  const bool live = c < N;
  float acc[kLpFB];
  lp_score_tile<SC>(Et, N, H, E, ldE, Rel, ldR, head, c, live, nfb,
                [&](int fi, int64_t &anchor, int64_t &rel) {
                  const int64_t a = queries[2 * (q0 + fi)];
                  anchor = a < 0 ? 0 : a >= N ? N - 1 : a;  // (ids are the caller's contract; never a read past E)
                  rel = queries[2 * (q0 + fi) + 1];
                },
                s_a, s_b, acc);
#pragma unroll
  for (int i = 0; i < kLpFB; ++i) {
    uint64_t key = 0;
    if (i < nfb && live) {
      const int64_t q = q0 + i;
      const bool masked = excl_ptr && in_sorted(excl_idx, excl_ptr[q], excl_ptr[q + 1], (int32_t)c);
      if (!masked) key = topk_key(acc[i], c);
    }
    s_key[i][threadIdx.x] = key;
  }
  topk_sort_tile(s_key, nfb);
  for (int e = threadIdx.x; e < nfb * k; e += kLpTB) {
    const int i = e / k, j = e - i * k;
    part[((q0 + i) * ntiles + blockIdx.x) * k + j] = s_key[i][j];
  }
}

// The type-constrained tiles (TypedQueries: queries grouped by relation on the host).  One block per work item {query
// tile, candidate tile}: at most kLpFB queries of ONE relation against kLpTB positions of that relation's slot on the
// asked side, candidate c = cand_idx[slot begin + position] scored by lp_score_tile with that c (the rank kernels'
// bits).  part[(order[q] * maxtiles + candidate tile) * k + j]: the lists sit under the CALLER'S query index, so the
// merge writes the rows in the caller's order.  A slot's candidates rise, and the key carries the node id: ties still go
// to the lower id.
template <int SC>
__global__ __launch_bounds__(kLpTB) void k_typed_topk_tiles(
    const float *__restrict__ Et, int64_t N, int H, const float *__restrict__ E, int64_t ldE,
    const float *__restrict__ Rel, int64_t ldR, const int64_t *__restrict__ queries, int64_t nq, int head_,
    const int64_t *__restrict__ order, const int64_t *__restrict__ tile_ptr, const int32_t *__restrict__ tile_rel,
    int64_t num_tiles, const int32_t *__restrict__ work, const int64_t *__restrict__ cand_ptr,
    const int32_t *__restrict__ cand_idx, const int64_t *__restrict__ excl_ptr, const int32_t *__restrict__ excl_idx,
    int k, int64_t maxtiles, uint64_t *__restrict__ part) {
  __shared__ float s_a[kLpFB][kLpHT];
  __shared__ float s_b[kLpFB][kLpHT];
  __shared__ uint64_t s_key[kLpFB][kLpTB];
  const bool head = head_ != 0;
  const int64_t tile = work[2 * (int64_t)blockIdx.x], ctile = work[2 * (int64_t)blockIdx.x + 1];
  if (tile < 0 || tile >= num_tiles || ctile < 0 || ctile >= maxtiles) return;   // (block-uniform, before any barrier)
  const int64_t p0 = tile_ptr[tile], cnt = tile_ptr[tile + 1] - p0;
  if (p0 < 0 || cnt <= 0 || p0 + cnt > nq) return;
  const int nfb = (int)(cnt < kLpFB ? cnt : kLpFB);
  const int64_t slot = 2 * (int64_t)tile_rel[tile] + (head ? 1 : 0);
  const int64_t begin = cand_ptr[slot], len = cand_ptr[slot + 1] - begin;
  const int64_t pos = ctile * kLpTB + threadIdx.x;
  const bool live = pos < len;
  int64_t c = live ? (int64_t)cand_idx[begin + pos] : 0;
  c = c < 0 ? 0 : c >= N ? N - 1 : c;
  float acc[kLpFB];
  lp_score_tile<SC>(Et, N, H, E, ldE, Rel, ldR, head, c, live, nfb,
                    [&](int fi, int64_t &anchor, int64_t &rel) {
                      const int64_t q = order[p0 + fi];
                      const int64_t a = queries[2 * q];
                      anchor = a < 0 ? 0 : a >= N ? N - 1 : a;
                      rel = queries[2 * q + 1];
                    },
                    s_a, s_b, acc);
#pragma unroll
  for (int i = 0; i < kLpFB; ++i) {
    uint64_t key = 0;
    if (i < nfb && live) {
      const int64_t q = order[p0 + i];
      const bool masked = excl_ptr && in_sorted(excl_idx, excl_ptr[q], excl_ptr[q + 1], (int32_t)c);
      if (!masked) key = topk_key(acc[i], c);
    }
    s_key[i][threadIdx.x] = key;
  }
  topk_sort_tile(s_key, nfb);
  for (int e = threadIdx.x; e < nfb * k; e += kLpTB) {
    const int i = e / k, j = e - i * k;
    part[(order[p0 + i] * maxtiles + ctile) * k + j] = s_key[i][j];
  }
}

// one block of max(K, 64) threads per query, K = the power of two >= k.  Query q owns `ntiles` lists of k keys, of which
// the first q_tiles[q] are written (NULL: all of them)
__global__ __launch_bounds__(kTopkMax) void k_topk_merge(const uint64_t *__restrict__ part, int64_t ntiles,
                                                         const int32_t *__restrict__ q_tiles, int k, int K,
                                                         int64_t *__restrict__ out_idx, float *__restrict__ out_score) {
  __shared__ uint64_t buf[2 * kTopkMax];  // [0, K): the best so far, descending; [K, 2K): the next list, ascending
  const int64_t q = blockIdx.x;
  const int t = threadIdx.x;
  const uint64_t *lists = part + q * ntiles * k;
  if (q_tiles) {
    const int64_t mine = q_tiles[q];
    ntiles = mine < 0 ? 0 : mine < ntiles ? mine : ntiles;
  }
  if (t < K) buf[t] = 0;
  uint64_t next = (t < k && ntiles > 0) ? lists[t] : 0;
  for (int64_t tile = 0; tile < ntiles; ++tile) {
    if (t < K) buf[2 * K - 1 - t] = next;
    if (tile + 1 < ntiles && t < k) next = lists[(tile + 1) * k + t];  // in flight across the merge
    for (int stride = K; stride > 0; stride >>= 1) {
      __syncthreads();
      if (t < K) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const uint64_t a = buf[lo], b = buf[hi];
        if (a < b) {
          buf[lo] = b;
          buf[hi] = a;
        }
      }
    }
    __syncthreads();
  }
  if (t < k) {
    const uint64_t key = buf[t];
    const uint32_t o = (uint32_t)(key >> 32);
    const uint32_t u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
    out_idx[q * k + t] = key ? (int64_t)(uint32_t)~(uint32_t)key : -1;
    out_score[q * k + t] = key ? __uint_as_float(u) : -INFINITY;
  }
}

inline int64_t et_bytes(int64_t N, int32_t H) { return ((int64_t)sizeof(float) * H * N + 7) / 8 * 8; }

}  // namespace
}  // namespace mrgcn

using namespace mrgcn;

extern "C" int64_t mrgcn_distmult_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k);

namespace {
template <int SC>
int topk_run(const char *who_, const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                        const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *excl_ptr,
                        const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes, int64_t *out_idx,
                        float *out_score, void *stream) {
  const std::string who(who_);
  MRGCN_REQUIRE(k >= 1 && k <= kTopkMax, who + ": k must be in [1, 256]");
  MRGCN_REQUIRE(num_queries >= 0 && num_queries < ((int64_t)1 << 31), who + ": 0 <= queries < 2^31");
  if (num_queries == 0) return MRGCN_OK;
  MRGCN_REQUIRE(E && Rel && queries && out_idx && out_score && workspace && H > 0 && num_nodes > 0 &&
                    num_nodes < ((int64_t)1 << 31) && (head == 0 || head == 1),
                who + ": bad argument");
  MRGCN_REQUIRE((excl_ptr == nullptr) == (excl_idx == nullptr),
                who + ": give both exclusion arrays (ptr, idx) or neither");
  MRGCN_REQUIRE(workspace_bytes >= mrgcn_distmult_topk_workspace(num_nodes, H, num_queries, k),
                who + ": workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float *Et = (float *)workspace;
  uint64_t *part = (uint64_t *)((char *)workspace + et_bytes(num_nodes, H));
  MRGCN_HIP_TRY(lp_transpose(E, ldE, num_nodes, H, Et, st));
  const int64_t ntiles = (num_nodes + kLpTB - 1) / kLpTB;
  // (a grid's y extent ends at 65 535 query tiles: more queries go out in several launches)
  const int64_t per_launch = (int64_t)65535 * kLpFB;
  for (int64_t q0 = 0; q0 < num_queries; q0 += per_launch) {
    const int64_t n = std::min(per_launch, num_queries - q0);
    dim3 grid((unsigned)ntiles, (unsigned)((n + kLpFB - 1) / kLpFB));
    k_topk_tiles<SC><<<grid, kLpTB, 0, st>>>(Et, num_nodes, H, E, ldE, Rel, ldR, queries + 2 * q0, n, head,
                                         excl_ptr ? excl_ptr + q0 : nullptr, excl_idx, k, ntiles,
                                         part + q0 * ntiles * k);
  }
  int K = 1;
  while (K < k) K <<= 1;
  k_topk_merge<<<(unsigned)num_queries, std::max(K, kWave), 0, st>>>(part, ntiles, nullptr, k, K, out_idx, out_score);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}
}  // namespace

namespace {
inline int64_t typed_tiles(int64_t max_slot) { return std::max<int64_t>(1, (max_slot + kLpTB - 1) / kLpTB); }

inline int64_t typed_topk_bytes(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k, int64_t max_slot) {
  if (num_nodes <= 0 || num_nodes >= ((int64_t)1 << 31) || H <= 0 || num_queries < 0 ||
      num_queries >= ((int64_t)1 << 31) || k < 1 || k > kTopkMax || max_slot < 0 || max_slot > num_nodes)
    return -1;
  // Et [H, N] floats (to 8 bytes) | tile lists [nq, candidate tiles of the LONGEST SLOT, k] 64-bit keys
  return et_bytes(num_nodes, H) + (int64_t)sizeof(uint64_t) * num_queries * typed_tiles(max_slot) * k;
}

template <int SC>
int typed_topk_run(const char *who_, const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR,
                   int32_t H, const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *order,
                   const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                   int64_t num_work, const int32_t *q_tiles, const int64_t *cand_ptr, const int32_t *cand_idx,
                   int64_t max_slot, const int64_t *excl_ptr, const int32_t *excl_idx, int32_t k, void *workspace,
                   int64_t workspace_bytes, int64_t *out_idx, float *out_score, void *stream) {
  const std::string who(who_);
  MRGCN_REQUIRE(k >= 1 && k <= kTopkMax, who + ": k must be in [1, 256]");
  MRGCN_REQUIRE(num_queries >= 0 && num_queries < ((int64_t)1 << 31), who + ": 0 <= queries < 2^31");
  if (num_queries == 0) return MRGCN_OK;
  MRGCN_REQUIRE(E && Rel && queries && out_idx && out_score && workspace && H > 0 && num_nodes > 0 &&
                    num_nodes < ((int64_t)1 << 31) && (head == 0 || head == 1),
                who + ": bad argument");
  MRGCN_REQUIRE(order && tile_ptr && tile_rel && q_tiles && cand_ptr && cand_idx && num_tiles >= 0 &&
                    num_tiles < ((int64_t)1 << 31) && num_work >= 0 && num_work < ((int64_t)1 << 31) &&
                    (work || num_work == 0) && max_slot >= 0 && max_slot <= num_nodes,
                who + ": grouping (order, tile_ptr, tile_rel, work, q_tiles) and candidate lists (cand_ptr, cand_idx)");
  MRGCN_REQUIRE((excl_ptr == nullptr) == (excl_idx == nullptr),
                who + ": give both exclusion arrays (ptr, idx) or neither");
  MRGCN_REQUIRE(workspace_bytes >= typed_topk_bytes(num_nodes, H, num_queries, k, max_slot),
                who + ": workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float *Et = (float *)workspace;
  uint64_t *part = (uint64_t *)((char *)workspace + et_bytes(num_nodes, H));
  MRGCN_HIP_TRY(lp_transpose(E, ldE, num_nodes, H, Et, st));
  const int64_t maxtiles = typed_tiles(max_slot);
  if (num_work > 0) {
    k_typed_topk_tiles<SC><<<(unsigned)num_work, kLpTB, 0, st>>>(Et, num_nodes, H, E, ldE, Rel, ldR, queries,
                                                                 num_queries, head, order, tile_ptr, tile_rel,
                                                                 num_tiles, work, cand_ptr, cand_idx, excl_ptr,
                                                                 excl_idx, k, maxtiles, part);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  int K = 1;
  while (K < k) K <<= 1;
  k_topk_merge<<<(unsigned)num_queries, std::max(K, kWave), 0, st>>>(part, maxtiles, q_tiles, k, K, out_idx,
                                                                     out_score);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}
}  // namespace

extern "C" {

int64_t mrgcn_distmult_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k) {
  if (num_nodes <= 0 || num_nodes >= ((int64_t)1 << 31) || H <= 0 || num_queries < 0 ||
      num_queries >= ((int64_t)1 << 31) || k < 1 || k > kTopkMax)
    return -1;
  // Et [H, N] floats (to 8 bytes) | tile lists [nq, candidate tiles, k] 64-bit keys
  const int64_t ntiles = (num_nodes + kLpTB - 1) / kLpTB;
  return et_bytes(num_nodes, H) + (int64_t)sizeof(uint64_t) * num_queries * ntiles * k;
}

int mrgcn_distmult_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                        const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *excl_ptr,
                        const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes, int64_t *out_idx,
                        float *out_score, void *stream) {
  return topk_run<kLpDistMult>("distmult_topk", E, ldE, num_nodes, Rel, ldR, H, queries, num_queries, head, excl_ptr,
                               excl_idx, k, workspace, workspace_bytes, out_idx, out_score, stream);
}

// The ComplEx twins (Trouillon et al. 2016): the same contract and workspace; scores are the ComplEx rank kernel's, bit
// for bit (lp_score.hpp: one body).
int64_t mrgcn_complex_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k) {
  return H % 2 == 0 ? mrgcn_distmult_topk_workspace(num_nodes, H, num_queries, k) : -1;
}

int mrgcn_complex_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                       const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *excl_ptr,
                       const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes, int64_t *out_idx,
                       float *out_score, void *stream) {
  MRGCN_REQUIRE(H > 0 && H % 2 == 0, "complex_topk: H must be even (H / 2 complex numbers per row)");
  return topk_run<kLpComplEx>("complex_topk", E, ldE, num_nodes, Rel, ldR, H, queries, num_queries, head, excl_ptr,
                              excl_idx, k, workspace, workspace_bytes, out_idx, out_score, stream);
}

// The type-constrained twins (TypedQueries): the k best nodes of the query relation's slot on the asked side.
int64_t mrgcn_distmult_typed_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k,
                                            int64_t max_slot) {
  return typed_topk_bytes(num_nodes, H, num_queries, k, max_slot);
}

int mrgcn_distmult_typed_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                              const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *order,
                              const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                              int64_t num_work, const int32_t *q_tiles, const int64_t *cand_ptr,
                              const int32_t *cand_idx, int64_t max_slot, const int64_t *excl_ptr,
                              const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                              int64_t *out_idx, float *out_score, void *stream) {
  return typed_topk_run<kLpDistMult>("distmult_typed_topk", E, ldE, num_nodes, Rel, ldR, H, queries, num_queries, head,
                                     order, tile_ptr, tile_rel, num_tiles, work, num_work, q_tiles, cand_ptr, cand_idx,
                                     max_slot, excl_ptr, excl_idx, k, workspace, workspace_bytes, out_idx, out_score,
                                     stream);
}

int64_t mrgcn_complex_typed_topk_workspace(int64_t num_nodes, int32_t H, int64_t num_queries, int32_t k,
                                           int64_t max_slot) {
  return H % 2 == 0 ? typed_topk_bytes(num_nodes, H, num_queries, k, max_slot) : -1;
}

int mrgcn_complex_typed_topk(const float *E, int64_t ldE, int64_t num_nodes, const float *Rel, int64_t ldR, int32_t H,
                             const int64_t *queries, int64_t num_queries, int32_t head, const int64_t *order,
                             const int64_t *tile_ptr, const int32_t *tile_rel, int64_t num_tiles, const int32_t *work,
                             int64_t num_work, const int32_t *q_tiles, const int64_t *cand_ptr,
                             const int32_t *cand_idx, int64_t max_slot, const int64_t *excl_ptr,
                             const int32_t *excl_idx, int32_t k, void *workspace, int64_t workspace_bytes,
                             int64_t *out_idx, float *out_score, void *stream) {
  MRGCN_REQUIRE(H > 0 && H % 2 == 0, "complex_typed_topk: H must be even (H / 2 complex numbers per row)");
  return typed_topk_run<kLpComplEx>("complex_typed_topk", E, ldE, num_nodes, Rel, ldR, H, queries, num_queries, head,
                                    order, tile_ptr, tile_rel, num_tiles, work, num_work, q_tiles, cand_ptr, cand_idx,
                                    max_slot, excl_ptr, excl_idx, k, workspace, workspace_bytes, out_idx, out_score,
                                    stream);
}

}  // extern "C"
