// Rank lists in LDS: the mechanics shared by the exact top-k finish kernels of dense.hip and
// sparse.hip. A list is a pair of arrays, (double key, int64 ordinal) per entry, ranked by
// (key desc, ordinal asc) with armi::lds_sort_rank_desc; unused slots hold the empty entry, which
// ranks behind every real one, so a sorted list is its real entries followed by its empty ones.
// Everything here is called by every thread of the workgroup.
#pragma once

#include <limits>

#include "armi_common.h"

namespace armi {

// The empty entry.
constexpr double kNegInfD = -std::numeric_limits<double>::infinity();
constexpr int64_t kNoOrd = std::numeric_limits<int64_t>::max();

// Empty entries over [from, to) of key / ord. No barrier.
__device__ __forceinline__ void fill_empty(double* key, int64_t* ord, int from, int to) {
  for (int e = from + (int)threadIdx.x; e < to; e += (int)blockDim.x) {
    key[e] = kNegInfD;
    ord[e] = kNoOrd;
  }
}

// The score written for a key: the dense kernels' key is 2^24 |q| cos, the sparse kernels' key is
// the score itself (no multiply: the product by 1.0 is not shared on purpose, the two stay the
// expressions their oracles compute).
struct ScoreTimes {
  double iq;
  __device__ __forceinline__ float operator()(double key) const { return (float)(key * iq); }
};
struct ScoreIsKey {
  __device__ __forceinline__ float operator()(double key) const { return (float)key; }
};

// The sorted [0, k) of key / ord as query q's outputs: scores, ids (-1 for an empty slot), rank
// keys (out_rank may be null) and the number of real entries. One slot per thread; there is no
// barrier and no reduction inside: the real entries of a sorted list come first, so the thread
// that holds the last of them (or slot 0 of an all-empty list) knows the count. The call follows
// the sort's trailing barrier. The flag word is the caller's.
template <typename Score>
__device__ __forceinline__ void write_top_k(const double* key, const int64_t* ord, int q, int k,
                                            Score score, float* __restrict__ out_scores,
                                            int64_t* __restrict__ out_ids,
                                            double* __restrict__ out_rank,
                                            int32_t* __restrict__ out_count) {
  for (int c = threadIdx.x; c < k; c += (int)blockDim.x) {
    const size_t o = (size_t)q * k + c;
    const bool v = ord[c] != kNoOrd;
    out_scores[o] = v ? score(key[c]) : -std::numeric_limits<float>::infinity();
    out_ids[o] = v ? ord[c] : -1;
    if (out_rank) out_rank[o] = v ? key[c] : kNegInfD;
    if (v ? (c + 1 == k || ord[c + 1] == kNoOrd) : c == 0) out_count[q] = v ? c + 1 : 0;
  }
}

// A loader brings a run of an incoming sequence into LDS: load(t0, m, key, ord) stores entries
// t0 .. t0 + m - 1 of the sequence at key / ord [0, m), an entry that does not rank as the empty
// entry, and touches no other slot. It is called by every thread, so a loader may spread a run over
// the threads, the waves (one dot product per wave) or groups of rows (exact_keys8) as it likes.

// m <= n incoming entries ranked at once: key / ord [0, n) sorted, n the power of two that holds
// max(m, keep) entries. The caller's previous use of [0, n) is over (a barrier) before the call.
template <typename Load>
__device__ __forceinline__ void rank_chunk(double* key, int64_t* ord, int m, int keep,
                                           Load&& load) {
  const int n = pow2_at_least(m > keep ? m : keep);
  load((int64_t)0, m, key, ord);
  fill_empty(key, ord, m, n);
  lds_sort_rank_desc(key, ord, n);
}

// The best `chunk` (a power of two) of `total` incoming entries, streamed through key / ord
// [0, 2 chunk): [0, chunk) holds the best so far, the loader brings the next run into
// [chunk, 2 chunk), and one sort of both halves per round leaves the best in front again. A
// sequence of at most one chunk is ranked once, in the lower half, as rank_chunk does (keep <=
// chunk); the loader still has one call site. On return [0, max(keep, min(total, chunk))) is
// sorted; as for rank_chunk, the caller's previous use of the arrays is over before the call.
template <typename Load>
__device__ __forceinline__ void merge_stream(double* key, int64_t* ord, int chunk, int keep,
                                             int64_t total, Load&& load) {
  const bool once = total <= chunk;  // workgroup-uniform
  const int at = once ? 0 : chunk;
  if (!once) fill_empty(key, ord, 0, chunk);
  int64_t t0 = 0;
  do {
    const int64_t left = total - t0;
    const int m = left < chunk ? (left > 0 ? (int)left : 0) : chunk;
    const int n = once ? pow2_at_least(m > keep ? m : keep) : 2 * chunk;
    // The previous round's sort is done with the upper half: its trailing barrier is what lets
    // this round overwrite [chunk, 2 chunk). Round 0 writes slots nobody has touched, and the
    // sort's leading barrier orders its stores and the fill of [0, chunk) before the first compare.
    load(t0, m, key + at, ord + at);
    fill_empty(key, ord, at + m, n);
    lds_sort_rank_desc(key, ord, n);
    t0 += chunk;
  } while (t0 < total);
}

// ---- row lists (armi_dense_rowlist_topk / armi_sparse_rowlist_topk) ----
// Rows per workgroup of a row-list call's chunk kernel, and entries per half of its merge.
constexpr int kRowlistChunk = 512;

// Chunks a list of len rows spans.
__host__ __device__ inline int64_t rowlist_chunks(int64_t len) {
  return len > 0 ? (len + kRowlistChunk - 1) / kRowlistChunk : 0;
}
// Chunk columns of a call's grid (and chunk lists per query in its workspace): at least one, so
// that an empty list is answered too.
inline int rowlist_grid_chunks(int64_t max_list_rows) {
  const int64_t c = rowlist_chunks(max_list_rows);
  return c > 1 ? (int)c : 1;
}

// Query q's row list: rows list_rows[lo .. lo + len), len cut to max_list_rows. A query naming no
// list (q_list[q] outside [0, n_lists)) ranks nothing: len == 0.
struct RowSpan {
  int64_t lo, len;
};
__device__ __forceinline__ RowSpan rowlist_span(const int64_t* __restrict__ list_ptr,
                                                const int32_t* __restrict__ q_list, int n_lists,
                                                int64_t max_list_rows, int q) {
  const int l = q_list[q];
  const bool listed = l >= 0 && l < n_lists;
  const int64_t lo = listed ? list_ptr[l] : 0;
  const int64_t len = listed ? min<int64_t>(list_ptr[l + 1] - lo, max_list_rows) : 0;
  return {lo, len};
}

}  // namespace armi
