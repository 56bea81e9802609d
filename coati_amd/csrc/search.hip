// Embedding-library search (include/coati_search.h): the k best rows of a bf16 library [N, E] for each of Q queries, by
// alpha * dot(q, row) + bias[row], score descending, row index ascending among equal scores.  No score is ever written to memory: one
// streaming kernel computes them on the matrix cores and keeps every query's k best in LDS, a second one merges the slices' lists.
//
// search_topk_kernel, grid = (tiles of 16 NP queries) x (S slices of the library), 4 waves; the tiles of one slice are neighbours in launch
// order, so that a slice read from HBM for one tile is found in the caches by the others:
//  * library rows are the M side of v_mfma_f32_16x16x32_bf16 and queries its N side: the result map (column = lane & 15, row =
//    4 (lane >> 4) + register) gives a lane four scores of ONE query per panel, which it filters against that query's threshold;
//  * the query tile's B fragments are loaded once and stay in registers (NP panels x E / 32 steps x 4 VGPRs); a wave streams 16-row
//    slabs of the library as 16-B loads per lane, the next slab's (and its bias) in flight under the current one's MFMAs.  One iteration
//    of the workgroup is 4 slabs = SEARCH_ROWS_IT rows, taken in ascending row order;
//  * LDS holds per query `cap` candidates as 64-bit keys (order-preserving score key << 32 | ~row: a larger key is a better candidate
//    and no two are equal), a count and a threshold (-inf at first).  A lane appends a score iff it is > the threshold, strictly: the
//    threshold is the k-th best of rows that all have SMALLER indices, so an equal score correctly loses;
//  * cap = k + 2 SEARCH_ROWS_IT.  An iteration adds at most SEARCH_ROWS_IT candidates to a query, and a compaction (to <= k) runs after
//    every iteration that left some count above cap - SEARCH_ROWS_IT: an append can never run past its buffer and no candidate is ever
//    dropped for lack of room, whatever the data;
//  * whether to compact is decided by ALL threads from one LDS word read after a barrier (two words, by iteration parity, so that one
//    barrier per iteration is enough); the trip count is the slice's, the same for every wave.  No barrier is under a lane- or
//    wave-dependent condition;
//  * a compaction pass takes the queries that are at least half way to that mark (count > k + SEARCH_ROWS_IT / 2) and leaves the others
//    as they are -- their thresholds stay valid, only less tight: at 64 queries the passes are set off by different queries at different
//    times, and a pass then ranks the lists that are worth it rather than all of them;
//  * a compaction ranks a query's candidates by counting (one wave per query, <= 4 candidates per lane against a broadcast read of each
//    key) and keeps the k best in rank order, so what is written out -- part[q][slice][0 .. k-1], padded with (-inf, -1) -- does not
//    depend on the order in which the LDS atomics landed.
// Rows >= N (ragged last slab, last slice) are read from a clamped address and masked to -inf after the MFMA; queries >= Q are zero
// fragments that are neither filtered nor stored.
//
// search_merge_kernel, one workgroup per query: the samplers' radix select (decode_dev.h) over the query's S * k partial scores.
// Candidate position order is (slice, rank) = ascending row index among equal scores, so the select's "index ascending" is the tie rule.
#include "decode_dev.h"

#define SEARCH_ROWS_IT 64
#define SEARCH_E_MAX 512
#define SEARCH_MERGE_MAX 30720   // S * k: the merge's row of keys in 120 KiB of LDS
#define SEARCH_DEVICE_SLOTS 512  // workgroups that fill the device: 256 CUs, two workgroups each where the LDS allows

typedef float search_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long search_key_t;

__device__ __forceinline__ search_key_t search_key(float s, int row) {
  return ((search_key_t)f2key(s) << 32) | (search_key_t)(~(unsigned)row);
}

// The k best of every query's candidates, in rank order at the front of its buffer; count and threshold follow.  Wave w takes the
// queries w, w + 4, ...; nothing here crosses waves, the caller's barriers separate it from the appends.  In the loop only the queries
// with more than k + SEARCH_ROWS_IT / 2 candidates are taken (every query above cap - SEARCH_ROWS_IT = k + SEARCH_ROWS_IT is one of them);
// FINAL: every list, also one of <= k candidates (the write-out needs them all in order).
template <bool FINAL>
__device__ __forceinline__ void search_compact(search_key_t* sbuf, int* s_cnt, float* s_thr, int nq, int cap, int k, int wave, int lane) {
  for (int ql = wave; ql < nq; ql += 4) {
    const int n = s_cnt[ql];
    if (FINAL ? n == 0 : n <= k + SEARCH_ROWS_IT / 2) continue;   // (n is the wave's: one LDS word)
    search_key_t* b = sbuf + ql * cap;
    search_key_t mine[4];
    int rank[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      mine[i] = e < n ? b[e] : 0ull;
      rank[i] = 0;
    }
    for (int j = 0; j < n; ++j) {
      const search_key_t kj = b[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) rank[i] += kj > mine[i] ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();   // every read of the buffer above, every write below
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (lane + 64 * i < n && rank[i] < k) {
        b[rank[i]] = mine[i];
        if (rank[i] == k - 1) s_thr[ql] = key2f((unsigned)(mine[i] >> 32));
      }
    }
    if (lane == 0) s_cnt[ql] = n < k ? n : k;
  }
}

template <int KSMAX, int NP>
__global__ __launch_bounds__(256) void search_topk_kernel(const bf16_t* __restrict__ lib, long long N, int E, const float* __restrict__ bias,
                                                          const bf16_t* __restrict__ q, int Q, int k, float alpha, int S, long long slice_rows,
                                                          int cap, float* __restrict__ part_score, int* __restrict__ part_row) {
  extern __shared__ search_key_t sbuf[];   // [16 NP][cap]
  __shared__ int s_cnt[16 * NP];
  __shared__ float s_thr[16 * NP];
  __shared__ int s_flag[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4), nq = 16 * np;
  const long long r_begin = (long long)slice * slice_rows, r_end = min(N, r_begin + slice_rows);
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + SEARCH_ROWS_IT - 1) / SEARCH_ROWS_IT) : 0;

  // the query tile: B[k = 32 s + 8 g + j][column = col] of panel p
  bf16x8 bq[NP][KSMAX];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && qi < Q) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[p][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
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

    search_f32x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = search_f32x4{0.f, 0.f, 0.f, 0.f};
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
        const bool stored = q0 + ql < Q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sc = alpha * acc[p][r] + bc[r];
          sc += 0.0f;   // -0 -> +0: the two must tie
          if (stored && sc > thr) {
            const int slot = atomicAdd(&s_cnt[ql], 1);   // < cap: the count was <= cap - SEARCH_ROWS_IT when this iteration began
            sbuf[ql * cap + slot] = search_key(sc, row0 + r);
            if (slot + 1 > cap - SEARCH_ROWS_IT) s_flag[it & 1] = 1;
          }
        }
      }
    }
    __syncthreads();
    const int full = s_flag[it & 1];   // read by every thread between two barriers with no write to it: workgroup-uniform
    if (full) {
      search_compact<false>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
      __syncthreads();
      if (tid == 0) s_flag[it & 1] = 0;   // (this word's next use is two iterations on, behind the next iteration's barrier)
    }
  }

  search_compact<true>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
  __syncthreads();
  for (int i = tid; i < nq * k; i += 256) {
    const int ql = i / k, r = i - ql * k;
    if (q0 + ql >= Q) continue;
    const long long o = ((long long)(q0 + ql) * S + slice) * k + r;
    const bool have = r < s_cnt[ql];
    const search_key_t key = sbuf[ql * cap + r];
    part_score[o] = have ? key2f((unsigned)(key >> 32)) : -INFINITY;
    part_row[o] = have ? (int)~(unsigned)key : -1;
  }
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
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX, "search_topk: k=%d outside 1 .. %d", k, TOPK_MAX);
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH_E_MAX && E % 32 == 0, "search_topk: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH_E_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "search_topk: N=%lld outside 1 .. 2^31 - 1", N);
  COATI_CHECK_SHAPE(Q >= 1, "search_topk: Q=%d < 1", Q);
  COATI_CHECK_SHAPE(S >= 1 && (long long)S * k <= SEARCH_MERGE_MAX, "search_topk: S=%d slices of k=%d exceed S * k <= %d", S, k, SEARCH_MERGE_MAX);
  return COATI_OK;
}

template <int KSMAX, int NP>
static int search_launch(const bf16_t* lib, long long N, int E, const float* bias, const bf16_t* q, int Q, int k, float alpha, int S,
                         float* part_score, int* part_row, hipStream_t s) {
  const int cap = k + 2 * SEARCH_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = (size_t)16 * NP * cap * sizeof(search_key_t);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(search_topk_kernel<KSMAX, NP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       16 * NP * (TOPK_MAX + 2 * SEARCH_ROWS_IT) * (int)sizeof(search_key_t));
    if (e != hipSuccess) {
      coati_set_error("search_topk: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  // slices of whole iterations; a slice past the end of the library (S > N / SEARCH_ROWS_IT) writes padding only
  const long long slice_rows = (N + (long long)S * SEARCH_ROWS_IT - 1) / ((long long)S * SEARCH_ROWS_IT) * SEARCH_ROWS_IT;
  hipLaunchKernelGGL((search_topk_kernel<KSMAX, NP>), dim3(cdiv(Q, 16 * NP), S), dim3(256), lds, s, lib, N, E, bias, q, Q, k, alpha, S,
                     slice_rows, cap, part_score, part_row);
  COATI_LAUNCH_CHECK("search_topk");
  return COATI_OK;
}

int launch_search_topk(const bf16_t* lib, long long N, int E, const float* bias, const bf16_t* q, int Q, int k, float alpha, int S,
                       float* part_score, int* part_row, float* out_score, long long* out_row, hipStream_t s) {
  COATI_CHECK_ARG(lib && q && part_score && part_row && out_score && out_row, "search_topk: null operand");
  COATI_TRY(search_check(N, E, Q, k, S));
  if (E <= 256)
    COATI_TRY((search_launch<8, 4>(lib, N, E, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  else
    COATI_TRY((search_launch<16, 2>(lib, N, E, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(search_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       SEARCH_MERGE_MAX * 4);
    if (e != hipSuccess) {
      coati_set_error("search_topk: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(search_merge_kernel, dim3(Q), dim3(256), (size_t)S * k * 4, s, part_score, part_row, S * k, k, out_score, out_row);
  COATI_LAUNCH_CHECK("search_merge");
  return COATI_OK;
}

// The number of slices launch_search_topk is given by default: enough workgroups to fill the device at this Q (tiles of 64 queries),
// no slice shorter than one workgroup iteration, S * k within the merge's row.  Host arithmetic only.
int search_slices(long long N, int Q, int k) {
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX && N >= 1 && N < (1ll << 31) && Q >= 1, "search_slices: N=%lld Q=%d k=%d out of range", N, Q, k);
  const long long tiles = ((long long)Q + 63) / 64;
  const long long by_rows = (N + SEARCH_ROWS_IT - 1) / SEARCH_ROWS_IT, by_merge = SEARCH_MERGE_MAX / k;
  long long S = (SEARCH_DEVICE_SLOTS + tiles - 1) / tiles;
  S = S < by_rows ? S : by_rows;
  S = S < by_merge ? S : by_merge;
  return (int)(S > 1 ? S : 1);
}
