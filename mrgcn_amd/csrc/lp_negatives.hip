// Keyed, filtered negatives for the link-prediction decoder, at any rate, on the device.
//
// The reference corrupts 20 % of a batch's positives, half at the head and half at the tail, with nodes of the batch,
// and never looks whether a corrupted triple is a known fact (mrgcn/tasks/link_prediction.py:247-264;
// mrgcn_corrupt_triples_i64 in distmult.hip is that scheme).  What differs here: EVERY fact gets `rate` negatives, the
// replacement is drawn from a candidate set the caller names (all entities, typically), and a draw that equals the end
// it replaces or that makes a known fact is refused and drawn again, up to MRGCN_NEG_MAX_ATTEMPTS times.
//
//   mrgcn_negatives_draw_i64   negative k = i * rate + j of fact i: attempt a = 0 .. 7 takes the Philox4x32-10 block
//                              (philox.hpp) of counter (k lo, (k >> 32) | (a << 24), position lo, position hi) under
//                              key (seed lo, seed hi ^ "NEGS"), picks candidate (x:y * n_cand) >> 64 and looks the
//                              corrupted triple's key up in the sorted key array; the first accepted attempt is written.
//                              Seed and position live in device memory; a one-thread launch behind the draw moves the
//                              position, so a replayed hipGraph draws fresh negatives at every replay.
//   mrgcn_negatives_draw_typed_i64   the same draw with the candidates of the fact's relation and side: slot 2 p
//                              (tails) / 2 p + 1 (heads) of a CSR of node lists (TypedCandidates).
//
// A one-shot grid: a thread owns one negative and leaves.  No atomics, no shared state: the result is a function of the
// arguments and the two state words, whatever the grid.  (mrgcn_amd/host.py: negatives_draw is the bit-exact mirror.)
#include "common.hpp"
#include "philox.hpp"

namespace mrgcn {
namespace {

constexpr int kTB = 256;
constexpr uint32_t kNegTag = 0x4E454753u;  // keeps this stream apart from node dropout's under the same seed

// Is `key` among the n > 0 ascending keys?  The trip count depends on n alone, so a wave walks the levels in step; each
// level is one dependent 8-byte read (the first levels are the same few lines for every thread, the whole array — 2.5 MB
// at FB15k-237 — sits in L2), hidden by the other waves of the CU.  Reads stay inside [0, n).
__device__ __forceinline__ bool key_known(const int64_t *__restrict__ keys, int64_t n, int64_t key) {
  int64_t base = 0, len = n;
  while (len > 1) {
    const int64_t half = len >> 1;
    base += keys[base + half] <= key ? half : 0;
    len -= half;
  }
  return keys[base] == key;
}

__global__ void __launch_bounds__(kTB) k_negatives_draw(const int64_t *__restrict__ facts, int64_t total, int32_t rate,
                                                        const int64_t *__restrict__ cand, int64_t n_cand,
                                                        const int64_t *__restrict__ to_global,
                                                        const int64_t *__restrict__ keys, int64_t n_known, int64_t N,
                                                        int64_t R, int32_t side, const int64_t *__restrict__ state,
                                                        int64_t *__restrict__ out, uint8_t *__restrict__ unresolved) {
  const int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (k >= total) return;
  const int64_t i = rate == 1 ? k : k / rate;
  const uint64_t seed = (uint64_t)state[0], pos = (uint64_t)state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ kNegTag;
  const int64_t s = facts[3 * i], p = facts[3 * i + 1], o = facts[3 * i + 2];
  const bool filter = keys != nullptr && n_known > 0;
  int64_t gs = s, go = o;
  if (filter && to_global) {
    gs = to_global[s];
    go = to_global[o];
  }
  bool head = side == 2;
  int64_t pick = 0;
  bool refused = true;
  for (uint32_t a = 0; a < MRGCN_NEG_MAX_ATTEMPTS && refused; ++a) {
    const U4 r = philox4x32_10(U4{(uint32_t)k, (uint32_t)((uint64_t)k >> 32) | (a << 24), (uint32_t)pos,
                                  (uint32_t)(pos >> 32)}, k0, k1);
    if (a == 0 && side == 0) head = (r.z & 1u) != 0;
    const uint64_t h = ((uint64_t)r.x << 32) | r.y;
    const int64_t c = (int64_t)__umul64hi(h, (uint64_t)n_cand);   // < n_cand
    pick = cand ? cand[c] : c;
    refused = pick == (head ? s : o);
    if (!refused && filter) {
      const int64_t gp = to_global ? to_global[pick] : pick;
      refused = key_known(keys, n_known, head ? (gp * R + p) * N + go : (gs * R + p) * N + gp);
    }
  }
  out[3 * k] = head ? pick : s;
  out[3 * k + 1] = p;
  out[3 * k + 2] = head ? o : pick;
  if (unresolved) unresolved[k] = refused ? 1 : 0;
}

// The type-constrained draw (Krompass, Baier, Tresp, ISWC 2015): the replacement of relation p's tail comes from slot
// 2 p of a CSR over 2 R slots (the relation's range), that of its head from slot 2 p + 1 (its domain).  The counter, the
// key, the side bit and the refusals are k_negatives_draw's; only the pick differs: idx[ptr[slot] + ((h * len) >> 64)].
// With every slot 0 .. N - 1 the pick is (h * N) >> 64 itself: the untyped draw, bit for bit.  An empty slot (the host
// refuses to build a sampler over one) reads nothing: the end stands and the negative is flagged.
__global__ void __launch_bounds__(kTB) k_negatives_draw_typed(const int64_t *__restrict__ facts, int64_t total,
                                                              int32_t rate, const int64_t *__restrict__ cand_ptr,
                                                              const int32_t *__restrict__ cand_idx,
                                                              const int64_t *__restrict__ keys, int64_t n_known,
                                                              int64_t N, int64_t R, int32_t side,
                                                              const int64_t *__restrict__ state,
                                                              int64_t *__restrict__ out,
                                                              uint8_t *__restrict__ unresolved) {
  const int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (k >= total) return;
  const int64_t i = rate == 1 ? k : k / rate;
  const uint64_t seed = (uint64_t)state[0], pos = (uint64_t)state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ kNegTag;
  const int64_t s = facts[3 * i], p = facts[3 * i + 1], o = facts[3 * i + 2];
  const bool filter = keys != nullptr && n_known > 0;
  const bool p_ok = p >= 0 && p < R;    // (a relation outside the lists has no slot: flagged, nothing read)
  bool head = side == 2;
  int64_t pick = 0, begin = 0, len = 0;
  bool refused = true;
  for (uint32_t a = 0; a < MRGCN_NEG_MAX_ATTEMPTS && refused; ++a) {
    const U4 r = philox4x32_10(U4{(uint32_t)k, (uint32_t)((uint64_t)k >> 32) | (a << 24), (uint32_t)pos,
                                  (uint32_t)(pos >> 32)}, k0, k1);
    if (a == 0) {
      if (side == 0) head = (r.z & 1u) != 0;
      if (p_ok) {
        begin = cand_ptr[2 * p + (head ? 1 : 0)];
        len = cand_ptr[2 * p + (head ? 1 : 0) + 1] - begin;
      }
    }
    if (len <= 0) {
      pick = head ? s : o;
      break;
    }
    const uint64_t h = ((uint64_t)r.x << 32) | r.y;
    const int64_t c = (int64_t)__umul64hi(h, (uint64_t)len);   // < len
    pick = cand_idx[begin + c];
    refused = pick == (head ? s : o);
    if (!refused && filter) refused = key_known(keys, n_known, head ? (pick * R + p) * N + o : (s * R + p) * N + pick);
  }
  out[3 * k] = head ? pick : s;
  out[3 * k + 1] = p;
  out[3 * k + 2] = head ? o : pick;
  if (unresolved) unresolved[k] = refused ? 1 : 0;
}

__global__ void k_negatives_advance(int64_t *__restrict__ state) { state[1] = state[1] + 1; }

}  // namespace
}  // namespace mrgcn

extern "C" {

int mrgcn_negatives_draw_i64(const int64_t *facts, int64_t n, int32_t rate, const int64_t *cand, int64_t n_cand,
                             const int64_t *to_global, const int64_t *known_keys, int64_t n_known, int64_t num_nodes,
                             int64_t num_relations, int32_t side, int64_t *state, int64_t *out, uint8_t *unresolved,
                             void *stream) {
  MRGCN_REQUIRE(facts && state && out, "NULL");
  MRGCN_REQUIRE(n >= 0 && rate >= 1, "n >= 0, rate >= 1");
  MRGCN_REQUIRE(n_cand >= 1, "empty candidate set");
  MRGCN_REQUIRE(n_known >= 0 && (side == 0 || side == 1 || side == 2), "n_known / side");
  MRGCN_REQUIRE(n < (((int64_t)1 << 56) + rate - 1) / rate, "n * rate < 2^56");
  MRGCN_REQUIRE(num_nodes >= 1 && num_relations >= 1 && num_relations <= INT64_MAX / num_nodes &&
                    num_nodes * num_relations <= INT64_MAX / num_nodes,
                "num_nodes * num_relations * num_nodes < 2^63");
  const int64_t total = n * rate;
  MRGCN_REQUIRE(total < ((int64_t)1 << 31) * mrgcn::kTB, "too many negatives for one grid");
  hipStream_t st = (hipStream_t)stream;
  if (total > 0) {
    mrgcn::k_negatives_draw<<<dim3((unsigned)((total + mrgcn::kTB - 1) / mrgcn::kTB)), dim3(mrgcn::kTB), 0, st>>>(
        facts, total, rate, cand, n_cand, to_global, known_keys, n_known, num_nodes, num_relations, side, state, out,
        unresolved);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  mrgcn::k_negatives_advance<<<dim3(1), dim3(1), 0, st>>>(state);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

int mrgcn_negatives_draw_typed_i64(const int64_t *facts, int64_t n, int32_t rate, const int64_t *cand_ptr,
                                   const int32_t *cand_idx, const int64_t *known_keys, int64_t n_known,
                                   int64_t num_nodes, int64_t num_relations, int32_t side, int64_t *state, int64_t *out,
                                   uint8_t *unresolved, void *stream) {
  MRGCN_REQUIRE(facts && state && out && cand_ptr && cand_idx, "NULL");
  MRGCN_REQUIRE(n >= 0 && rate >= 1, "n >= 0, rate >= 1");
  MRGCN_REQUIRE(n_known >= 0 && (side == 0 || side == 1 || side == 2), "n_known / side");
  MRGCN_REQUIRE(n < (((int64_t)1 << 56) + rate - 1) / rate, "n * rate < 2^56");
  MRGCN_REQUIRE(num_nodes >= 1 && num_relations >= 1 && num_relations <= INT64_MAX / num_nodes &&
                    num_nodes * num_relations <= INT64_MAX / num_nodes,
                "num_nodes * num_relations * num_nodes < 2^63");
  const int64_t total = n * rate;
  MRGCN_REQUIRE(total < ((int64_t)1 << 31) * mrgcn::kTB, "too many negatives for one grid");
  hipStream_t st = (hipStream_t)stream;
  if (total > 0) {
    mrgcn::k_negatives_draw_typed<<<dim3((unsigned)((total + mrgcn::kTB - 1) / mrgcn::kTB)), dim3(mrgcn::kTB), 0,
                                    st>>>(facts, total, rate, cand_ptr, cand_idx, known_keys, n_known, num_nodes,
                                          num_relations, side, state, out, unresolved);
    MRGCN_HIP_TRY(hipGetLastError());
  }
  mrgcn::k_negatives_advance<<<dim3(1), dim3(1), 0, st>>>(state);
  MRGCN_HIP_TRY(hipGetLastError());
  return MRGCN_OK;
}

}  // extern "C"
