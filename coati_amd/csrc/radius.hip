// Radius search (include/coati_radius.h): every row of a bf16 library [N, E] whose score alpha * dot(q, row) + bias[row] - sub[q] reaches
// the query's threshold, in CSR form.  The answer's size is known only after a scan, so the same kernel runs twice: a count pass writes
// counts [Q, S], the caller's prefix sum turns them into offsets, a fill pass computes the scores again and writes the hits.
//
// radius_kernel<KSMAX, NP, FILL>, grid = (tiles of 16 NP queries) x (S slices of the library), 4 waves -- the exact search's geometry
// (search.hip) and the exact search's stream: a workgroup loads its query tile's B fragments once, a wave streams 16-row slabs as 16-B
// loads per lane with the next slab in flight under the current one's MFMAs, one iteration of the workgroup is 4 slabs = TOPK_ROWS_IT rows
// in ascending row order.  The result map (column = lane & 15, row = 4 (lane >> 4) + register) gives a lane four rows of ONE query per
// panel.  The back end differs: a threshold filter in registers instead of the LDS top-k lists.
//  * the score lines -- the slab's addresses, the k-steps over E from zero accumulators, alpha * acc + bias, the + 0.0f -- MIRROR
//    topk_stream (topk_stream_dev.h) line by line, so that a (query, row) pair has the bits coati_search_topk gives it.  They are restated
//    here, not shared: lifting them into functions of that header moved the register allocation of the two kernels that include it;
//  * count pass: a lane counts its own hits in registers, no barrier in the loop; one reduction over the 4 waves x 4 lane groups at the end;
//  * fill pass: per panel four wave-wide ballots (one per register r) give every lane its query's hits in the wave as a 64-bit word y
//    with bit 16 g' + r = (lane col + 16 g', register r): ascending bit order is ascending row order.  The wave's popcount goes to one
//    byte of an LDS word per query (a wave has <= 16 hits per query and iteration), double-buffered by iteration parity, so one barrier
//    per iteration is enough: a word of parity p is written again two iterations on, behind the next iteration's barrier, which no wave
//    passes before all have read.  A hit's position is then running + (hits of lower waves) + (bits of y below mine): data alone, no
//    atomics, no dependence on S or on which wave ran first;
//  * every barrier is workgroup-uniform: the trip count comes from blockIdx, the arguments and global words (row_hi, counts) that every
//    thread reads alike;
//  * two uniform early exits.  A workgroup whose slice begins at or above the largest row_hi of its tile has nothing to do (its slice is
//    also cut at that bound): a self-join with row_hi[i] = i is a triangle, not a square.  A fill workgroup whose tile has no hit in its
//    slice -- it knows from counts -- returns before loading anything.
// Rows >= the slice's end are read from an address clamped to row N - 1 and masked by a bias of -inf.  A fill never writes outside
// [offsets, offsets + counts) of its (query, slice).
#include <climits>
#include <type_traits>

#include "../../include/coati_radius.h"
#include "search_host.h"

#define RADIUS_E_MAX 512
#define RADIUS_S_MAX 65535        // gridDim.y

__device__ __forceinline__ int radius_bytesum(unsigned x) { return (int)((x * 0x01010101u) >> 24); }   // (of four bytes that sum to < 256)

template <int KSMAX, int NP, bool FILL>
__global__ __launch_bounds__(256) void radius_kernel(const bf16_t* __restrict__ lib, long long N, int E, const float* __restrict__ bias,
                                                     const bf16_t* __restrict__ q, int Q, float alpha, const float* __restrict__ sub, int clamp0,
                                                     const float* __restrict__ thr, const int* __restrict__ row_hi, int S, long long slice_rows,
                                                     std::conditional_t<FILL, const int*, int*> __restrict__ counts,
                                                     const long long* __restrict__ offsets, float* __restrict__ out_score,
                                                     long long* __restrict__ out_row) {
  __shared__ unsigned s_wc[FILL ? 2 * 16 * NP : 1];      // fill: [parity][query], byte w = wave w's hits of the iteration
  __shared__ int s_red[FILL ? 1 : 16 * 16 * NP];         // count: [wave][lane group][query]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4), nq = min(16 * np, Q - q0);
  const long long r_begin = (long long)slice * slice_rows;
  long long r_end = min(N, r_begin + slice_rows);

  // workgroup-uniform: the tile's largest row bound cuts the slice, and a fill with no hit to write has nothing to do
  long long hi_max = row_hi ? 0 : N;
  int any = 0;
  for (int j = 0; j < nq; ++j) {
    if (row_hi) hi_max = max(hi_max, (long long)row_hi[q0 + j]);
    if (FILL) any |= counts[(long long)(q0 + j) * S + slice];
  }
  r_end = min(r_end, hi_max);
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;
  if constexpr (FILL) {
    if (any == 0 || iters == 0) return;
  } else {
    if (iters == 0) {
      if (tid < nq) counts[(long long)(q0 + tid) * S + slice] = 0;
      return;
    }
  }

  // the query tile: B[k = 32 s + 8 g + j][column = col] of panel p, as search_topk_kernel loads it; a column without a query gets a zero
  // fragment and a row bound of 0: no row is below it
  bf16x8 bq[NP][KSMAX];
  float th[NP], sb[NP];
  unsigned rh[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
    const bool stored = qi < Q;
    th[p] = stored ? thr[qi] : INFINITY;
    sb[p] = stored && sub ? sub[qi] : 0.f;
    rh[p] = stored ? (row_hi ? (unsigned)max(row_hi[qi], 0) : (unsigned)INT_MAX) : 0u;
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[p][s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  int cnt[NP];              // count: the lane's own hits
  int run[NP], lim[NP];     // fill: the query's hits of the earlier iterations, and counts of (query, slice)
  long long off[NP];        // fill: offsets of (query, slice)
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    cnt[p] = run[p] = lim[p] = 0;
    off[p] = 0;
    if constexpr (FILL) {
      const int qi = q0 + 16 * p + col;
      if (qi < Q) {
        lim[p] = counts[(long long)qi * S + slice];
        off[p] = offsets[(long long)qi * S + slice];
      }
    }
  }

  // ---- the stream: mirrors topk_stream (topk_stream_dev.h) ----
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
  load_slab(0);

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

    // filter: the lane's four rows of each panel against its query's threshold and row bound; acc becomes the value reported
    const unsigned row0 = (unsigned)(r_begin + 16ll * (4 * it + wave)) + 4u * g;
    unsigned long long y[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      y[p] = 0ull;
      if (p < np) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sc = alpha * acc[p][r] + bc[r];
          sc += 0.0f;   // -0 -> +0: the two must tie
          // ---- end of the mirrored lines ----
          float v = sc - sb[p];
          if (clamp0) v = fminf(v, 0.f);
          const bool hit = sc > -INFINITY && v >= th[p] && row0 + r < rh[p];
          acc[p][r] = v;
          if constexpr (FILL)
            y[p] |= ((__builtin_amdgcn_ballot_w64(hit) >> col) & 0x0001000100010001ull) << r;
          else
            cnt[p] += hit ? 1 : 0;
        }
        if constexpr (FILL) {
          if (g == 0) reinterpret_cast<unsigned char*>(s_wc)[4 * ((it & 1) * 16 * NP + 16 * p + col) + wave] = (unsigned char)__popcll(y[p]);
        }
      }
    }
    if constexpr (FILL) {
      __syncthreads();
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (p < np) {
          const unsigned word = s_wc[(it & 1) * 16 * NP + 16 * p + col];
          const int total = radius_bytesum(word);
          if (total == 0) continue;
          const int before = run[p] + radius_bytesum(word & ((1u << (8 * wave)) - 1u));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int bit = 16 * g + r;
            if ((y[p] >> bit) & 1ull) {
              const int idx = before + __popcll(y[p] & ((1ull << bit) - 1ull));
              if (idx < lim[p]) {   // (always, with the counts and offsets of the header)
                out_row[off[p] + idx] = (long long)(row0 + r);
                out_score[off[p] + idx] = acc[p][r];
              }
            }
          }
          run[p] += total;
        }
      }
    }
  }

  if constexpr (!FILL) {
#pragma unroll
    for (int p = 0; p < NP; ++p) s_red[(4 * wave + g) * 16 * NP + 16 * p + col] = cnt[p];
    __syncthreads();
    if (tid < nq) {
      int n = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) n += s_red[i * 16 * NP + tid];
      counts[(long long)(q0 + tid) * S + slice] = n;
    }
  }
}

static int radius_check(const char* what, long long N, int E, int Q, int S) {
  COATI_CHECK_SHAPE(E >= 32 && E <= RADIUS_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, RADIUS_E_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "%s: N=%lld outside 1 .. 2^31 - 1", what, N);
  COATI_CHECK_SHAPE(Q >= 1, "%s: Q=%d < 1", what, Q);
  COATI_CHECK_SHAPE(S >= 1 && S <= RADIUS_S_MAX, "%s: S=%d outside 1 .. %d", what, S, RADIUS_S_MAX);
  return COATI_OK;
}

template <int KSMAX, int NP, bool FILL>
static int radius_launch(const char* what, const bf16_t* lib, long long N, int E, const float* bias, const bf16_t* q, int Q, float alpha,
                         const float* sub, int clamp0, const float* thr, const int* row_hi, int S,
                         std::conditional_t<FILL, const int*, int*> counts, const long long* offsets, float* out_score, long long* out_row,
                         hipStream_t s) {
  hipLaunchKernelGGL((radius_kernel<KSMAX, NP, FILL>), dim3(cdiv(Q, 16 * NP), S), dim3(256), 0, s, lib, N, E, bias, q, Q, alpha, sub, clamp0, thr,
                     row_hi, S, topk_slice_rows(N, S), counts, offsets, out_score, out_row);
  COATI_LAUNCH_CHECK(what);
  return COATI_OK;
}

int coati_radius_count(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, float alpha, const float* sub,
                       int clamp0, const float* thr, const int32_t* row_hi, int S, int32_t* counts, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "radius_count: lib is null");
  COATI_CHECK_ARG(q, "radius_count: q is null");
  COATI_CHECK_ARG(thr, "radius_count: thr is null");
  COATI_CHECK_ARG(counts, "radius_count: counts is null");
  COATI_TRY(radius_check("radius_count", N, E, Q, S));
  if (E <= 256)
    return radius_launch<8, 4, false>("radius_count", lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, nullptr, nullptr, nullptr, s);
  return radius_launch<16, 2, false>("radius_count", lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, nullptr, nullptr, nullptr, s);
}

int coati_radius_fill(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, float alpha, const float* sub,
                      int clamp0, const float* thr, const int32_t* row_hi, int S, const int32_t* counts, const int64_t* offsets,
                      float* out_score, int64_t* out_row, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "radius_fill: lib is null");
  COATI_CHECK_ARG(q, "radius_fill: q is null");
  COATI_CHECK_ARG(thr, "radius_fill: thr is null");
  COATI_CHECK_ARG(counts, "radius_fill: counts is null");
  COATI_CHECK_ARG(offsets, "radius_fill: offsets is null");
  COATI_CHECK_ARG(out_score, "radius_fill: out_score is null");
  COATI_CHECK_ARG(out_row, "radius_fill: out_row is null");
  COATI_TRY(radius_check("radius_fill", N, E, Q, S));
  if (E <= 256)
    return radius_launch<8, 4, true>("radius_fill", lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, LL(offsets), out_score,
                                     LL(out_row), s);
  return radius_launch<16, 2, true>("radius_fill", lib, N, E, bias, q, Q, alpha, sub, clamp0, thr, row_hi, S, counts, LL(offsets), out_score,
                                    LL(out_row), s);
}

// The number of slices the two passes are given by default: enough workgroups to fill the device at this Q (tiles of 64 queries), no
// slice shorter than one workgroup iteration, within the grid's y limit.  There is no merge, so no merge bound.  Host arithmetic only.
int coati_radius_slices(int64_t N, int Q) {
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31) && Q >= 1, "radius_slices: N=%lld Q=%d out of range", (long long)N, Q);
  const long long tiles = ((long long)Q + 63) / 64, by_rows = (N + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT;
  long long S = (TOPK_DEVICE_SLOTS + tiles - 1) / tiles;
  S = S < by_rows ? S : by_rows;
  S = S < RADIUS_S_MAX ? S : RADIUS_S_MAX;
  return (int)(S > 1 ? S : 1);
}
