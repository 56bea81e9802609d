// The streaming top-k body of the exact search (search.hip) and of the IVF scan (ivf.hip): the k best rows of a range [r_begin, r_end) of
// a bf16 library [N, E] for up to 16 NP queries, by alpha * dot(q, row) + bias[row], score descending, row index ascending among equal
// scores.  No score is ever written to memory: the scores are computed on the matrix cores and every query's k best stay in LDS.  Both
// kernels run THIS code, so a (query, row) score has the same bits in both: the k-steps over E, alpha * acc + bias and the -0 -> +0 step
// exist once.
//
// topk_stream, one workgroup of 4 waves, every thread of it:
//  * library rows are the M side of v_mfma_f32_16x16x32_bf16 and queries its N side: the result map (column = lane & 15, row =
//    4 (lane >> 4) + register) gives a lane four scores of ONE query per panel, which it filters against that query's threshold;
//  * the queries' B fragments are loaded once by the caller and stay in registers (NP panels x E / 32 steps x 4 VGPRs); a wave streams
//    16-row slabs of the library as 16-B loads per lane, the next slab's (and its bias) in flight under the current one's MFMAs.  One
//    iteration of the workgroup is 4 slabs = TOPK_ROWS_IT rows, taken in ascending row order;
//  * LDS holds per query `cap` candidates as 64-bit keys (order-preserving score key << 32 | ~row: a larger key is a better candidate
//    and no two are equal), a count and a threshold (-inf at first).  A lane appends a score iff it is > the threshold, strictly: the
//    threshold is the k-th best of rows that all have SMALLER indices, so an equal score correctly loses;
//  * cap = k + 2 TOPK_ROWS_IT.  An iteration adds at most TOPK_ROWS_IT candidates to a query, and a compaction (to <= k) runs after
//    every iteration that left some count above cap - TOPK_ROWS_IT: an append can never run past its buffer and no candidate is ever
//    dropped for lack of room, whatever the data;
//  * whether to compact is decided by ALL threads from one LDS word read after a barrier (two words, by iteration parity, so that one
//    barrier per iteration is enough); the trip count is the row range's, which the caller gives every thread alike.  No barrier is
//    under a lane- or wave-dependent condition;
//  * a compaction pass takes the queries that are at least half way to that mark (count > k + TOPK_ROWS_IT / 2) and leaves the others
//    as they are -- their thresholds stay valid, only less tight: at 64 queries the passes are set off by different queries at different
//    times, and a pass then ranks the lists that are worth it rather than all of them;
//  * a compaction ranks a query's candidates by counting (one wave per query, <= 4 candidates per lane against a broadcast read of each
//    key) and keeps the k best in rank order, so what topk_write_out writes -- a query's slots 0 .. k-1, padded with (-inf, -1) -- does
//    not depend on the order in which the LDS atomics landed.
// Rows >= r_end (ragged last slab) are read from an address clamped to row N - 1 and masked to -inf after the MFMA; a column whose
// `stored` flag is off (no query there: the caller loaded a zero fragment) is neither filtered nor stored.
#pragma once
#include "decode_dev.h"

#define TOPK_ROWS_IT 64   // rows per workgroup iteration

typedef float topk_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long topk_key_t;

__device__ __forceinline__ topk_key_t topk_key(float s, int row) {
  return ((topk_key_t)f2key(s) << 32) | (topk_key_t)(~(unsigned)row);
}
__device__ __forceinline__ float topk_key_score(topk_key_t key) { return key2f((unsigned)(key >> 32)); }
__device__ __forceinline__ int topk_key_row(topk_key_t key) { return (int)~(unsigned)key; }

// The k best of every query's candidates, in rank order at the front of its buffer; count and threshold follow.  Wave w takes the
// queries w, w + 4, ...; nothing here crosses waves, the caller's barriers separate it from the appends.  In the loop only the queries
// with more than k + TOPK_ROWS_IT / 2 candidates are taken (every query above cap - TOPK_ROWS_IT = k + TOPK_ROWS_IT is one of them);
// FINAL: every list, also one of <= k candidates (the write-out needs them all in order).
template <bool FINAL>
__device__ __forceinline__ void topk_compact(topk_key_t* sbuf, int* s_cnt, float* s_thr, int nq, int cap, int k, int wave, int lane) {
  for (int ql = wave; ql < nq; ql += 4) {
    const int n = s_cnt[ql];
    if (FINAL ? n == 0 : n <= k + TOPK_ROWS_IT / 2) continue;   // (n is the wave's: one LDS word)
    topk_key_t* b = sbuf + ql * cap;
    topk_key_t mine[4];
    int rank[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      mine[i] = e < n ? b[e] : 0ull;
      rank[i] = 0;
    }
    for (int j = 0; j < n; ++j) {
      const topk_key_t kj = b[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) rank[i] += kj > mine[i] ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();   // every read of the buffer above, every write below
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (lane + 64 * i < n && rank[i] < k) {
        b[rank[i]] = mine[i];
        if (rank[i] == k - 1) s_thr[ql] = topk_key_score(mine[i]);
      }
    }
    if (lane == 0) s_cnt[ql] = n < k ? n : k;
  }
}

// Rows [r_begin, r_end) of lib [N, E] (both bounds workgroup-uniform; an empty range leaves empty lists) against the B fragments
// bq[p][s] = B[k = 32 s + 8 g + j][column = col] of panels p < np; stored[p]: the lane's column of panel p holds a query.  On return (behind a
// barrier) query ql's min(k, candidates) best keys are sbuf[ql * cap ..] in rank order and s_cnt[ql] is their number.  sbuf [16 NP][cap],
// s_cnt and s_thr [16 NP], s_flag [2] are LDS that the reset below overwrites: a caller that read them before (the last call's lists)
// puts a barrier between that and this call.
template <int KSMAX, int NP>
__device__ __forceinline__ void topk_stream(const bf16_t* __restrict__ lib, long long N, int E, const float* __restrict__ bias,
                                            const bf16x8 (&bq)[NP][KSMAX], int np, const bool (&stored)[NP], long long r_begin, long long r_end,
                                            float alpha, int k, int cap, topk_key_t* sbuf, int* s_cnt, float* s_thr, int* s_flag) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5, nq = 16 * np;
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;
  if (tid < 16 * NP) {
    s_cnt[tid] = 0;
    s_thr[tid] = -INFINITY;
  }
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();

  // a wave's slab of iteration it: rows r_begin + 16 (4 it + wave) .. + 15; A[row = col][k = 32 s + 8 g + j].  A row >= N is read at
  // row N - 1 (inside the allocation) and masked after the MFMA; bn = the bias of the lane's four result rows (-inf: masked)
  uint4 an[KSMAX];
  float bn[4];
#pragma unroll
  for (int s = 0; s < KSMAX; ++s) an[s] = make_uint4(0u, 0u, 0u, 0u);
  auto load_slab = [&](int it) {
    const long long slab = r_begin + 16ll * (4 * it + wave);
    const long long row = min(slab + col, N - 1);
    const uint4* src = reinterpret_cast<const uint4*>(lib + row * E + 8 * g);
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      if (s < ks) an[s] = src[4 * s];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long br = slab + 4 * g + r;
      bn[r] = br < r_end ? (bias ? bias[br] : 0.f) : -INFINITY;
    }
  };
  if (iters > 0) load_slab(0);

  for (int it = 0; it < iters; ++it) {
    uint4 ac[KSMAX];
    float bc[4];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) ac[s] = an[s];
#pragma unroll
    for (int r = 0; r < 4; ++r) bc[r] = bn[r];
    if (it + 1 < iters) load_slab(it + 1);

    topk_f32x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < ks) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
          if (p < np) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ac[s]), bq[p][s], acc[p], 0, 0, 0);
      }
    }

    // filter: the lane's four rows of each panel against its query's threshold
    const int row0 = (int)(r_begin + 16ll * (4 * it + wave)) + 4 * g;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (p < np) {
        const int ql = 16 * p + col;
        const float thr = s_thr[ql];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sc = alpha * acc[p][r] + bc[r];
          sc += 0.0f;   // -0 -> +0: the two must tie
          if (stored[p] && sc > thr) {
            const int slot = atomicAdd(&s_cnt[ql], 1);   // < cap: the count was <= cap - TOPK_ROWS_IT when this iteration began
            sbuf[ql * cap + slot] = topk_key(sc, row0 + r);
            if (slot + 1 > cap - TOPK_ROWS_IT) s_flag[it & 1] = 1;
          }
        }
      }
    }
    __syncthreads();
    const int full = s_flag[it & 1];   // read by every thread between two barriers with no write to it: workgroup-uniform
    if (full) {
      topk_compact<false>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
      __syncthreads();
      if (tid == 0) s_flag[it & 1] = 0;   // (this word's next use is two iterations on, behind the next iteration's barrier)
    }
  }

  topk_compact<true>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
  __syncthreads();
}

// After topk_stream: queries 0 .. nq - 1 of the workgroup write their k slots, query ql's at part_*[o0 + ql * q_stride ..], in rank order:
// (score, row_of(the key's row)), then (-inf, -1).
template <class RowOf>
__device__ __forceinline__ void topk_write_out(const topk_key_t* sbuf, const int* s_cnt, int cap, int k, int nq, long long o0, long long q_stride,
                                               RowOf row_of, float* __restrict__ part_score, int* __restrict__ part_row) {
  for (int i = threadIdx.x; i < nq * k; i += 256) {
    const int ql = i / k, r = i - ql * k;
    const long long o = o0 + ql * q_stride + r;
    const bool have = r < s_cnt[ql];
    const topk_key_t key = sbuf[ql * cap + r];
    part_score[o] = have ? topk_key_score(key) : -INFINITY;
    part_row[o] = have ? row_of(topk_key_row(key)) : -1;
  }
}
