// Radius search over inverted lists (include/coati_ivf_radius.h): every row of a query's probed lists whose score reaches the query's
// threshold, in CSR form over the (query, list) pairs.  ivf_scan_kernel's work items (ivf.hip) around radius_kernel's stream and filter
// (radius.hip) with one query panel; neither of the two is touched, both are restated here as radius.hip restates topk_stream.
//
// ivf_radius_kernel<KSMAX, FILL>, 4 waves.  The operands are the scan's: lib / ids / bias / list_off in list order, the (query, list)
// pairs sorted by (list, query) as pair_q / pair_off, the work-item table item_off.  A work item is (list l, group of <= 16 of its
// pairs, segment of seg_rows of its positions), numbered segment-major; a workgroup takes items blockIdx.x, + gridDim.x, ... and finds an
// item's list by bisection of item_off.  Per item it gathers the group's queries through pair_q into B fragments (a column past the
// group's last pair, or with a query outside 0 .. Q - 1, is a zero fragment with a row bound of 0: it has no hit) and streams the
// segment's 16-row slabs with the next slab in flight; one iteration of the workgroup is 4 slabs = TOPK_ROWS_IT positions in ascending
// order.
//  * the score lines -- the slab's addresses, the k-steps over E from zero accumulators, alpha * acc + bias, the + 0.0f -- MIRROR
//    topk_stream (topk_stream_dev.h) line by line, then - sub[q] and fminf(., 0) under clamp0 as in radius.hip: a (query, row) pair has
//    the bits coati_search_topk, coati_ivf_scan and coati_radius_* give it;
//  * a hit: score above -inf, value >= thr[q], and with row_hi ids[position] < row_hi[q].  The ids of a slab are prefetched with its
//    bias only when row_hi is given; the fill reads ids[position] again for the hits it writes;
//  * count pass: a lane counts its own hits in registers, no barrier in the stream; one reduction over the 4 waves x 4 lane groups per
//    item writes counts[pair, segment].  The caller zero-fills counts: a (pair, segment) that no item covers, or whose item is skipped,
//    stays 0;
//  * fill pass: radius_kernel<.., true>'s placement.  Four wave-wide ballots give every lane its query's hits in the wave as a 64-bit
//    word with bit 16 g' + r = (lane group g', register r): ascending bit order is ascending position order.  The wave's popcount goes
//    to one byte of an LDS word per query, double-buffered by iteration parity, one barrier per iteration.  A hit lands at
//    offsets[pair, segment] + (hits of the earlier iterations) + (hits of lower waves) + (bits below mine): data alone, no atomics, no
//    dependence on blocks, seg_rows or which workgroup ran the item;
//  * the parity words outlive an item: its last iteration's word may be the next item's first.  A barrier ends every item that ran, so
//    no wave writes the next item's word 0 while another still reads this item's (ivf_scan_kernel has the same barrier after its
//    write-out).  The count pass needs it for s_red likewise;
//  * every trip count and every skip is workgroup-uniform: the item's list, pair range, row range, group and segment come from the same
//    global words (item_off, pair_off, list_off) in every thread; the two early exits below are ballots over the 16 columns, which
//    every wave holds alike (lanes of equal col read the same words), so every wave takes the same branch;
//  * two uniform early exits.  A fill item whose group has no count in its segment has nothing to write.  An item whose segment's first
//    id is at or above every row bound of its group has no hit: ids ascend inside a list (the header's precondition) -- the self-join
//    with row_hi = the query's own row skips the later part of every list.
// Positions >= the segment's end are read from an address clamped to position M - 1 and masked by a bias of -inf.  A fill never writes
// outside [offsets, offsets + counts) of its (pair, segment).
#include <climits>
#include <type_traits>

#include "../../include/coati_ivf_radius.h"
#include "topk_stream_dev.h"

__device__ __forceinline__ int ivf_radius_bytesum(unsigned x) { return (int)((x * 0x01010101u) >> 24); }   // (of four bytes that sum to < 256)

template <int KSMAX, bool FILL>
__global__ __launch_bounds__(256) void ivf_radius_kernel(const bf16_t* __restrict__ lib, const int* __restrict__ ids, const float* __restrict__ bias,
                                                         const int* __restrict__ list_off, long long M, int E, int L, const bf16_t* __restrict__ q,
                                                         int Q, const int* __restrict__ pair_q, const int* __restrict__ pair_off,
                                                         const int* __restrict__ item_off, long long P, float alpha, const float* __restrict__ sub,
                                                         int clamp0, const float* __restrict__ thr, const int* __restrict__ row_hi, int seg_rows,
                                                         int segs, std::conditional_t<FILL, const int*, int*> __restrict__ counts,
                                                         const long long* __restrict__ offsets, float* __restrict__ out_score,
                                                         long long* __restrict__ out_row) {
  __shared__ unsigned s_wc[FILL ? 2 * 16 : 1];      // fill: [parity][query], byte w = wave w's hits of the iteration
  __shared__ int s_red[FILL ? 1 : 16 * 16];         // count: [wave][lane group][query]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const long long items = item_off[L];

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int l = item_owner(item_off, L, item);   // (lists without items share their successor's entry)
    const long long p_begin = min(max((long long)pair_off[l], 0ll), P), p_end = min(max((long long)pair_off[l + 1], p_begin), P);
    const long long l_begin = min(max((long long)list_off[l], 0ll), M), l_end = min(max((long long)list_off[l + 1], l_begin), M);
    const long long groups = (p_end - p_begin + 15) >> 4, j = item - item_off[l];
    if (groups < 1 || j < 0) continue;   // (not the documented table; every thread reads the same words: skipped by all)
    const long long sg = j / groups, pg = j - sg * groups;
    const long long r_begin = l_begin + sg * seg_rows, r_end = min(l_end, r_begin + seg_rows);
    if (sg >= segs || r_begin >= r_end) continue;
    const long long p0 = p_begin + 16 * pg;
    const int nq = (int)min(16ll, p_end - p0);
    const int iters = (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT);

    // the lane's column: its pair, query, threshold and row bound; a column without a query has a row bound of 0 -- no id is below it
    const long long slot = (p0 + col) * segs + sg;   // of counts / offsets [P, segs]
    int qi = -1;
    if (col < nq) qi = pair_q[p0 + col];
    const bool stored = qi >= 0 && qi < Q;
    const float th = stored ? thr[qi] : INFINITY;
    const float sb = stored && sub ? sub[qi] : 0.f;
    const unsigned rh = stored ? (row_hi ? (unsigned)max(row_hi[qi], 0) : (unsigned)INT_MAX) : 0u;
    int lim = 0;              // fill: counts of (pair, segment)
    long long off = 0;        // fill: offsets of (pair, segment)
    if constexpr (FILL) {
      if (col < nq) {
        lim = counts[slot];
        off = offsets[slot];
      }
      if (__builtin_amdgcn_ballot_w64(lim != 0) == 0ull) continue;   // nothing to write for this group in this segment
    }
    // ids ascend inside a list: a segment whose first id no column's bound exceeds has no hit (also: a group without any query)
    if (__builtin_amdgcn_ballot_w64((unsigned)ids[r_begin] < rh) == 0ull) continue;

    // the group's queries: B[k = 32 s + 8 g + j][column = col], as ivf_scan_kernel loads them
    bf16x8 bq[KSMAX];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[s] = __builtin_bit_cast(bf16x8, v);
    }

    int cnt = 0;              // count: the lane's own hits
    int run = 0;              // fill: the query's hits of the earlier iterations

    // ---- the stream: mirrors topk_stream (topk_stream_dev.h) ----
    // a wave's slab of iteration it: positions r_begin + 16 (4 it + wave) .. + 15; A[row = col][k = 32 s + 8 g + j].  A position >= M is
    // read at M - 1 (inside the allocation) and masked after the MFMA; bn = the bias of the lane's four result rows (-inf: masked),
    // idn = their original rows (read only under a row bound)
    uint4 an[KSMAX];
    float bn[4];
    int idn[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) an[s] = make_uint4(0u, 0u, 0u, 0u);
    auto load_slab = [&](int it) {
      const long long slab = r_begin + 16ll * (4 * it + wave);
      const long long row = min(slab + col, M - 1);
      const uint4* src = reinterpret_cast<const uint4*>(lib + row * E + 8 * g);
#pragma unroll
      for (int s = 0; s < KSMAX; ++s)
        if (s < ks) an[s] = src[4 * s];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long br = slab + 4 * g + r;
        bn[r] = br < r_end ? (bias ? bias[br] : 0.f) : -INFINITY;
        if (row_hi) idn[r] = ids[min(br, M - 1)];
      }
    };
    load_slab(0);

    for (int it = 0; it < iters; ++it) {
      uint4 ac[KSMAX];
      float bc[4];
      int idc[4];
#pragma unroll
      for (int s = 0; s < KSMAX; ++s) ac[s] = an[s];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bc[r] = bn[r];
        idc[r] = idn[r];
      }
      if (it + 1 < iters) load_slab(it + 1);

      topk_f32x4 acc = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KSMAX; ++s) {
        if (s < ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ac[s]), bq[s], acc, 0, 0, 0);
      }

      // filter: the lane's four positions against its query's threshold and row bound; acc becomes the value reported
      const int row0 = (int)(r_begin + 16ll * (4 * it + wave)) + 4 * g;
      unsigned long long y = 0ull;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sc = alpha * acc[r] + bc[r];
        sc += 0.0f;   // -0 -> +0: the two must tie
        // ---- end of the mirrored lines ----
        float v = sc - sb;
        if (clamp0) v = fminf(v, 0.f);
        const bool hit = sc > -INFINITY && v >= th && (unsigned)idc[r] < rh;
        acc[r] = v;
        if constexpr (FILL)
          y |= ((__builtin_amdgcn_ballot_w64(hit) >> col) & 0x0001000100010001ull) << r;
        else
          cnt += hit ? 1 : 0;
      }
      if constexpr (FILL) {
        if (g == 0) reinterpret_cast<unsigned char*>(s_wc)[4 * ((it & 1) * 16 + col) + wave] = (unsigned char)__popcll(y);
        __syncthreads();
        const unsigned word = s_wc[(it & 1) * 16 + col];
        const int total = ivf_radius_bytesum(word);
        if (total != 0) {
          const int before = run + ivf_radius_bytesum(word & ((1u << (8 * wave)) - 1u));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int bit = 16 * g + r;
            if ((y >> bit) & 1ull) {
              const int idx = before + __popcll(y & ((1ull << bit) - 1ull));
              if (idx < lim) {   // (always, with the counts and offsets of the header)
                out_row[off + idx] = (long long)ids[row0 + r];   // (a hit's position is one of r_begin .. r_end - 1 < M)
                out_score[off + idx] = acc[r];
              }
            }
          }
          run += total;
        }
      }
    }

    if constexpr (!FILL) {
      s_red[(4 * wave + g) * 16 + col] = cnt;
      __syncthreads();
      if (tid < nq) {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) n += s_red[i * 16 + tid];
        counts[(p0 + tid) * segs + sg] = n;
      }
    }
    __syncthreads();   // the next item's first parity word (fill) or sums (count), behind this item's reads of them
  }
}

// The checks both passes share under the name `what` -- coati_ivf_scan's limits (ivf_scan_grid, at k = 1) -- and its grid.
static int ivf_radius_grid(const char* what, long long M, int E, int L, int Q, long long P, int seg_rows, int segs, int blocks) {
  return ivf_scan_grid(what, M, E, L, Q, P, 1, seg_rows, segs, blocks);
}

template <int KSMAX, bool FILL>
static int ivf_radius_launch(const char* what, int grid, const bf16_t* lib, const int* ids, const float* bias, const int* list_off, long long M,
                             int E, int L, const bf16_t* q, int Q, const int* pair_q, const int* pair_off, const int* item_off, long long P,
                             float alpha, const float* sub, int clamp0, const float* thr, const int* row_hi, int seg_rows, int segs,
                             std::conditional_t<FILL, const int*, int*> counts, const long long* offsets, float* out_score, long long* out_row,
                             hipStream_t s) {
  hipLaunchKernelGGL((ivf_radius_kernel<KSMAX, FILL>), dim3(grid), dim3(256), 0, s, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off,
                     item_off, P, alpha, sub, clamp0, thr, row_hi, seg_rows, segs, counts, offsets, out_score, out_row);
  COATI_LAUNCH_CHECK(what);
  return COATI_OK;
}

int coati_ivf_radius_count(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                           const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P,
                           float alpha, const float* sub, int clamp0, const float* thr, const int32_t* row_hi, int seg_rows, int segs,
                           int32_t* counts, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "ivf_radius_count: lib is null");
  COATI_CHECK_ARG(ids, "ivf_radius_count: ids is null");
  COATI_CHECK_ARG(list_off, "ivf_radius_count: list_off is null");
  COATI_CHECK_ARG(q, "ivf_radius_count: q is null");
  COATI_CHECK_ARG(pair_q, "ivf_radius_count: pair_q is null");
  COATI_CHECK_ARG(pair_off, "ivf_radius_count: pair_off is null");
  COATI_CHECK_ARG(item_off, "ivf_radius_count: item_off is null");
  COATI_CHECK_ARG(thr, "ivf_radius_count: thr is null");
  COATI_CHECK_ARG(counts, "ivf_radius_count: counts is null");
  const int grid = ivf_radius_grid("ivf_radius_count", M, E, L, Q, P, seg_rows, segs, blocks);
  if (grid < 0) return grid;
  if (E <= 256)
    return ivf_radius_launch<8, false>("ivf_radius_count", grid, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub,
                                       clamp0, thr, row_hi, seg_rows, segs, counts, nullptr, nullptr, nullptr, s);
  return ivf_radius_launch<16, false>("ivf_radius_count", grid, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub,
                                      clamp0, thr, row_hi, seg_rows, segs, counts, nullptr, nullptr, nullptr, s);
}

int coati_ivf_radius_fill(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                          const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P,
                          float alpha, const float* sub, int clamp0, const float* thr, const int32_t* row_hi, int seg_rows, int segs,
                          const int32_t* counts, const int64_t* offsets, float* out_score, int64_t* out_row, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "ivf_radius_fill: lib is null");
  COATI_CHECK_ARG(ids, "ivf_radius_fill: ids is null");
  COATI_CHECK_ARG(list_off, "ivf_radius_fill: list_off is null");
  COATI_CHECK_ARG(q, "ivf_radius_fill: q is null");
  COATI_CHECK_ARG(pair_q, "ivf_radius_fill: pair_q is null");
  COATI_CHECK_ARG(pair_off, "ivf_radius_fill: pair_off is null");
  COATI_CHECK_ARG(item_off, "ivf_radius_fill: item_off is null");
  COATI_CHECK_ARG(thr, "ivf_radius_fill: thr is null");
  COATI_CHECK_ARG(counts, "ivf_radius_fill: counts is null");
  COATI_CHECK_ARG(offsets, "ivf_radius_fill: offsets is null");
  COATI_CHECK_ARG(out_score, "ivf_radius_fill: out_score is null");
  COATI_CHECK_ARG(out_row, "ivf_radius_fill: out_row is null");
  const int grid = ivf_radius_grid("ivf_radius_fill", M, E, L, Q, P, seg_rows, segs, blocks);
  if (grid < 0) return grid;
  if (E <= 256)
    return ivf_radius_launch<8, true>("ivf_radius_fill", grid, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub,
                                      clamp0, thr, row_hi, seg_rows, segs, counts, LL(offsets), out_score, LL(out_row), s);
  return ivf_radius_launch<16, true>("ivf_radius_fill", grid, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P, alpha, sub,
                                     clamp0, thr, row_hi, seg_rows, segs, counts, LL(offsets), out_score, LL(out_row), s);
}
