// Embedding-library search (include/coati_search.h): the k best rows of a bf16 library [N, E] for each of Q queries, by
// alpha * dot(q, row) + bias[row], score descending, row index ascending among equal scores.  No score is ever written to memory: one
// streaming kernel computes them on the matrix cores and keeps every query's k best in LDS, a second one merges the slices' lists.
//
// search_topk_kernel, grid = (tiles of 16 NP queries) x (S slices of the library), 4 waves; the tiles of one slice are neighbours in launch
// order, so that a slice read from HBM for one tile is found in the caches by the others.  A workgroup loads its query tile's B fragments
// (contiguous rows of q; queries >= Q are zero fragments that are neither filtered nor stored), runs topk_stream (topk_stream_dev.h: the
// result map, the strict >, why cap is safe, why every barrier is uniform, why the written order does not depend on atomic order) over
// its slice -- the slice's bounds come from blockIdx and the arguments, the same for every thread -- and writes part[q][slice][0 .. k-1],
// the row being the key's row.
//
// search_merge_kernel, one workgroup per query: the samplers' radix select (decode_dev.h) over the query's S * k partial scores.
// Candidate position order is (slice, rank) = ascending row index among equal scores, so the select's "index ascending" is the tie rule.
#include "../../include/coati_search.h"
#include "search_host.h"

#define SEARCH_E_MAX 512

template <int KSMAX, int NP>
__global__ __launch_bounds__(256) void search_topk_kernel(const bf16_t* __restrict__ lib, long long N, int E, const float* __restrict__ bias,
                                                          const bf16_t* __restrict__ q, int Q, int k, float alpha, int S, long long slice_rows,
                                                          int cap, float* __restrict__ part_score, int* __restrict__ part_row) {
  extern __shared__ topk_key_t sbuf[];   // [16 NP][cap]
  __shared__ int s_cnt[16 * NP];
  __shared__ float s_thr[16 * NP];
  __shared__ int s_flag[2];
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4);
  const long long r_begin = (long long)slice * slice_rows, r_end = min(N, r_begin + slice_rows);

  // the query tile: B[k = 32 s + 8 g + j][column = col] of panel p
  bf16x8 bq[NP][KSMAX];
  bool stored[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
    stored[p] = qi < Q;
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored[p]) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[p][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  topk_stream<KSMAX, NP>(lib, N, E, bias, bq, np, stored, r_begin, r_end, alpha, k, cap, sbuf, s_cnt, s_thr, s_flag);
  topk_write_out(sbuf, s_cnt, cap, k, min(16 * np, Q - q0), ((long long)q0 * S + slice) * k, (long long)S * k, [](int row) { return row; },
                 part_score, part_row);
}

// One workgroup per query: the k best of its S * k partial candidates (key descending, position ascending) with their library rows.
__global__ __launch_bounds__(256) void search_merge_kernel(const float* __restrict__ part_score, const int* __restrict__ part_row, int V, int k,
                                                           float* __restrict__ out_score, long long* __restrict__ out_row) {
  extern __shared__ unsigned keys[];   // [V]
  __shared__ TopkLds sm;
  const long long qi = blockIdx.x;
  topk_select_row(part_score + qi * V, V, k, keys, sm);
  const int tid = threadIdx.x;
  if (tid < k) {
    out_score[qi * k + tid] = key2f(sm.top_k[tid]);
    out_row[qi * k + tid] = part_row[qi * V + sm.top_i[tid]];   // (-1 where the score is the -inf padding)
  }
}

static int search_check(long long N, int E, int Q, int k, int S) {
  COATI_TRY(topk_check("search_topk", N, Q, k, S));
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH_E_MAX && E % 32 == 0, "search_topk: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH_E_MAX);
  return COATI_OK;
}

template <int KSMAX, int NP>
static int search_launch(const bf16_t* lib, long long N, int E, const float* bias, const bf16_t* q, int Q, int k, float alpha, int S,
                         float* part_score, int* part_row, hipStream_t s) {
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = (size_t)16 * NP * cap * sizeof(topk_key_t);
  COATI_TRY((max_dynamic_lds<search_topk_kernel<KSMAX, NP>>("search_topk", 16 * NP * (TOPK_MAX + 2 * TOPK_ROWS_IT) * (int)sizeof(topk_key_t))));
  hipLaunchKernelGGL((search_topk_kernel<KSMAX, NP>), dim3(cdiv(Q, 16 * NP), S), dim3(256), lds, s, lib, N, E, bias, q, Q, k, alpha, S,
                     topk_slice_rows(N, S), cap, part_score, part_row);
  COATI_LAUNCH_CHECK("search_topk");
  return COATI_OK;
}

int coati_search_topk(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, int k, float alpha, int S,
                      float* part_score, int32_t* part_row, float* out_score, int64_t* out_row, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib && q && part_score && part_row && out_score && out_row, "search_topk: null operand");
  COATI_TRY(search_check(N, E, Q, k, S));
  if (E <= 256)
    COATI_TRY((search_launch<8, 4>(lib, N, E, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  else
    COATI_TRY((search_launch<16, 2>(lib, N, E, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  return launch_search_merge(part_score, part_row, Q, S * k, k, out_score, LL(out_row), s);
}

// The merge alone, also for the stream kernels of other files that write the same partial lists (search8.hip, search4.hip, pq.hip):
// out [Q, k] from part [Q, V].
int launch_search_merge(const float* part_score, const int* part_row, int Q, int V, int k, float* out_score, long long* out_row, hipStream_t s) {
  COATI_CHECK_ARG(part_score && part_row && out_score && out_row, "search_merge: null operand");
  COATI_CHECK_SHAPE(Q >= 1 && k >= 1 && k <= TOPK_MAX && V >= k && V <= TOPK_MERGE_MAX, "search_merge: Q=%d V=%d k=%d out of range", Q, V, k);
  COATI_TRY(max_dynamic_lds<search_merge_kernel>("search_merge", TOPK_MERGE_MAX * 4));
  hipLaunchKernelGGL(search_merge_kernel, dim3(Q), dim3(256), (size_t)V * 4, s, part_score, part_row, V, k, out_score, out_row);
  COATI_LAUNCH_CHECK("search_merge");
  return COATI_OK;
}

// The number of slices coati_search_topk is given by default (topk_default_slices).  Host arithmetic only.
int coati_search_slices(int64_t N, int Q, int k) { return topk_default_slices("search_slices", N, Q, k); }
