// The bookkeeping of tasks/utils.py::EarlyStop (:64-81) on the device struct, shared by the kernels that record into it
// (early_stop.hip: k_early_stop_record, the four-value metrics row; lp_eval.hip: k_early_stop_record_row, a row of
// any width).  One thread runs it.
#pragma once

#include "common.hpp"

namespace mrgcn {

// Clears `improved`; false once `stop` is latched: epochs that run before the host notices leave no trace, so the
// caller then neither writes its metrics row nor books the record.
__device__ __forceinline__ bool early_stop_open(mrgcn_early_stop_state *__restrict__ st) {
  st->improved = 0;
  return !st->stop;
}

// Counts the record and decides (after the caller wrote its row to `records % rows`).
__device__ __forceinline__ void early_stop_book(mrgcn_early_stop_state *__restrict__ st,
                                                const float *__restrict__ score, double tolerance,
                                                int patience_default) {
  st->records += 1;
  if (st->delay > 0) {
    st->delay -= 1;
    return;
  }
  const double s = (double)*score;
  if (st->best_score < 0) {  // the first record that counts: no patience spent
    st->best_score = s;
    st->best_record = st->records;
    st->improved = 1;
    return;
  }
  st->patience -= 1;
  if (s + tolerance < st->best_score) {
    st->best_score = s;
    st->best_record = st->records;
    st->improved = 1;
    st->patience = patience_default;
  }
  if (st->patience <= 0) st->stop = 1;
}

}  // namespace mrgcn
