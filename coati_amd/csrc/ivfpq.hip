// IVF-PQ search (include/coati_ivfpq.h): inverted lists whose positions are stored as product-quantisation codes of the RESIDUAL, row minus
// its list's centre -- codes [M, E / 8] in list order under ONE set of code books [E / 8][256][8] bf16 shared by all lists, the bf16 centres
// [L, E] the coarse step already uses.  The row a position stands for is x_hat[p] = centre[l] + entry(codes[p]); a query scores only the
// positions of the lists it probes.  No score is ever written to memory, no result depends on the launch geometry.  The merge
// (ivf_merge_kernel of ivf.hip), the plan (coati_ivf_plan) and the exact re-scoring (search_rescore_kernel of search8.hip) are used as they are.
//
// ivfpq_scan_kernel<KSMAX>, 4 waves, one query panel of 16 pairs: ivf_scan_kernel's item loop (ivf.hip) around pq_stream (pq_stream_dev.h)
// with its START switch.  The probe table arrives inverted: the (query, list) pairs sorted by (list, query).  A work item is (list l, group
// of <= 16 of its pairs, segment of seg_rows of its rows), numbered segment-major; a workgroup takes items blockIdx.x, + gridDim.x, ...
// and finds an item's list by bisection of item_off.
//  * the whole code book (512 E bytes) is copied into LDS ONCE per workgroup, before the item loop and behind a barrier: the workgroups
//    are persistent over the items, so the default grid is at most one workgroup per CU and the copy is paid once per CU, not per slice
//    as in pq_topk_kernel.  LDS, all of it dynamic: the code book | the lists [16][cap] of 8-byte keys | counts | thresholds | flags;
//  * per item the group's queries are gathered through pair_q into B fragments (columns past the group's last pair, or with a query
//    outside 0 .. Q - 1, are zero fragments that are neither filtered nor stored).  ONE MFMA pass from a zero accumulator multiplies them
//    with the list's centre in all 16 rows of the A fragment -- lane (col, g) loads centre[32 s + 8 g .. + 7], the same 16 bytes for every
//    col: a broadcast -- which leaves q_col . centre in all four accumulator registers of the lane.  pq_stream starts every slab's
//    accumulator from that value and continues the chain with the E / 32 k-steps of the code-book entries.  The score alpha * acc +
//    bias[p], a zero canonicalised to +0, is therefore bit for bit what ivf_scan_kernel computes at width 2 E for the library row
//    [centre[l] | entry(codes[p])] against the query [q | q]: an MFMA's result element depends on its own A row and B column alone.  The
//    cost is E / 32 MFMAs and 2 E bytes per item;
//  * the stream's "row" is a position of codes here.  Its strict > stays the tie rule: the threshold is the k-th best of positions that
//    are all SMALLER, and inside a list a smaller position is a smaller original row (the header's precondition);
//  * positions >= the segment's end are read at min(position, M - 1) -- inside codes -- and masked by a -inf bias after the MFMA;
//  * every table word is clamped before it is used: p_begin <= p_end within 0 .. P, l_begin <= l_end within 0 .. M, l within 0 .. L - 1
//    (item_owner), so a position streamed is in 0 .. M - 1, a pair read in 0 .. P - 1 and a centre read in 0 .. L - 1 whatever the tables
//    hold.
// Why every barrier is workgroup-uniform: the trip count of the item loop is item_off[L], blockIdx.x and gridDim.x; an item's list, pair
// range, row range, group and segment are computed by every thread from the same global words and the arguments, so `continue` is taken by
// all threads or none; inside pq_stream the trip count is the segment's r_begin and r_end and whether to compact is read by all threads
// from one LDS word behind a barrier.  A column without a query only has a zero fragment and stored = false.  The barrier after the
// write-out puts the next item's reset of the counts behind this item's reads of them.
#include "../../include/coati_ivfpq.h"
#include "pq_stream_dev.h"
#include "search_host.h"

#define IVFPQ_E_MAX 256
#define IVFPQ_LDS_BYTES (160 * 1024)   // a CU's LDS, which one workgroup may take whole
#define IVFPQ_WORDS_BYTES (16 * 8 + 8)   // counts and thresholds [16], flags [2]
#define IVFPQ_GRID_MAX 256             // one workgroup per CU: each holds the code book

static inline size_t ivfpq_lds(int E, int k) { return (size_t)512 * E + (size_t)16 * (k + 2 * TOPK_ROWS_IT) * sizeof(topk_key_t) + IVFPQ_WORDS_BYTES; }

template <int KSMAX>
__global__ __launch_bounds__(256) void ivfpq_scan_kernel(const unsigned char* __restrict__ codes, const int* __restrict__ ids,
                                                         const float* __restrict__ bias, const int* __restrict__ list_off, long long M, int E,
                                                         int L, const bf16_t* __restrict__ centres, const bf16_t* __restrict__ codebook,
                                                         const bf16_t* __restrict__ q, int Q, const int* __restrict__ pair_q,
                                                         const int* __restrict__ pair_off, const int* __restrict__ item_off, long long P, int k,
                                                         float alpha, int seg_rows, int segs, int cap, float* __restrict__ part_score,
                                                         int* __restrict__ part_row) {
  extern __shared__ uint4 ivfpq_lds_base[];   // code book [E / 8][256] x 16 B | lists [16][cap] x 8 B | counts | thresholds | flags
  uint4* cb = ivfpq_lds_base;
  topk_key_t* sbuf = reinterpret_cast<topk_key_t*>(cb + 32 * E);
  int* s_cnt = reinterpret_cast<int*>(sbuf + 16 * cap);
  float* s_thr = reinterpret_cast<float*>(s_cnt + 16);
  int* s_flag = reinterpret_cast<int*>(s_thr + 16);
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const long long items = item_off[L];

  for (int i = tid; i < 32 * E; i += 256) cb[i] = reinterpret_cast<const uint4*>(codebook)[i];
  __syncthreads();

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

    // the group's queries: B[k = 32 s + 8 g + j][column = col]; the centre in every row of A: q_col . centre in all four registers
    int qi = -1;
    if (col < nq) qi = pair_q[p0 + col];
    const bool stored[1] = {qi >= 0 && qi < Q};
    bf16x8 bq[1][KSMAX];
    topk_f32x4 start[1] = {topk_f32x4{0.f, 0.f, 0.f, 0.f}};
    const uint4* csrc = reinterpret_cast<const uint4*>(centres + (long long)l * E + 8 * g);
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored[0]) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[0][s] = __builtin_bit_cast(bf16x8, v);
      if (s < ks) start[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, csrc[4 * s]), bq[0][s], start[0], 0, 0, 0);
    }
    pq_stream<KSMAX, 1, true>(codes, M, E, cb, bias, bq, 1, stored, r_begin, r_end, alpha, k, cap, sbuf, s_cnt, s_thr, s_flag, start);
    // (a stored position is one of r_begin .. r_end - 1 < M)
    topk_write_out(sbuf, s_cnt, cap, k, nq, (p0 * segs + sg) * k, (long long)segs * k, [&](int pos) { return ids[pos]; }, part_score, part_row);
    __syncthreads();   // the next item's reset of the counts, behind this one's reads
  }
}

static int ivfpq_check_E(const char* what, int E) {
  COATI_CHECK_SHAPE(E >= 32 && E <= IVFPQ_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, IVFPQ_E_MAX);
  return COATI_OK;
}

// The largest k of the scan at this E: 128 where the code book, the lists of 16 pairs at cap = k + 2 TOPK_ROWS_IT and the words fit the
// CU's 160 KiB, else 64 (E = 256: 128 KiB + 24 KiB + 136 B); a negative code for an E outside the limits
int coati_ivfpq_k_max(int E) {
  COATI_TRY(ivfpq_check_E("ivfpq_k_max", E));
  for (int k = TOPK_MAX; k >= 64; k /= 2)
    if (ivfpq_lds(E, k) <= IVFPQ_LDS_BYTES) return k;
  coati_set_error("ivfpq_k_max: no k fits E=%d", E);   // (not reached within the limits)
  return COATI_ESHAPE;
}

template <int KSMAX>
static int ivfpq_launch(const unsigned char* codes, const int* ids, const float* bias, const int* list_off, long long M, int E, int L,
                        const bf16_t* centres, const bf16_t* codebook, const bf16_t* q, int Q, const int* pair_q, const int* pair_off,
                        const int* item_off, long long P, int k, float alpha, int seg_rows, int segs, float* part_score, int* part_row, int grid,
                        hipStream_t s) {
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = ivfpq_lds(E, k);     // <= IVFPQ_LDS_BYTES: k <= coati_ivfpq_k_max(E)
  COATI_TRY(max_dynamic_lds<ivfpq_scan_kernel<KSMAX>>("ivfpq_scan", IVFPQ_LDS_BYTES));
  hipLaunchKernelGGL((ivfpq_scan_kernel<KSMAX>), dim3(grid), dim3(256), lds, s, codes, ids, bias, list_off, M, E, L, centres, codebook, q, Q, pair_q,
                     pair_off, item_off, P, k, alpha, seg_rows, segs, cap, part_score, part_row);
  COATI_LAUNCH_CHECK("ivfpq_scan");
  return COATI_OK;
}

int coati_ivfpq_scan(const uint8_t* codes, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                     const uint16_t* centres, const uint16_t* codebook, const uint16_t* q, int Q, const int32_t* pair_q,
                     const int32_t* pair_off, const int32_t* item_off, int64_t P, int k, float alpha, int seg_rows, int segs,
                     float* part_score, int32_t* part_row, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(codes, "ivfpq_scan: codes is null");
  COATI_CHECK_ARG(ids, "ivfpq_scan: ids is null");
  COATI_CHECK_ARG(bias, "ivfpq_scan: bias is null");
  COATI_CHECK_ARG(list_off, "ivfpq_scan: list_off is null");
  COATI_CHECK_ARG(centres, "ivfpq_scan: centres is null");
  COATI_CHECK_ARG(codebook, "ivfpq_scan: codebook is null");
  COATI_CHECK_ARG(q, "ivfpq_scan: q is null");
  COATI_CHECK_ARG(pair_q, "ivfpq_scan: pair_q is null");
  COATI_CHECK_ARG(pair_off, "ivfpq_scan: pair_off is null");
  COATI_CHECK_ARG(item_off, "ivfpq_scan: item_off is null");
  COATI_CHECK_ARG(part_score, "ivfpq_scan: part_score is null");
  COATI_CHECK_ARG(part_row, "ivfpq_scan: part_row is null");
  COATI_TRY(ivfpq_check_E("ivfpq_scan", E));
  int grid = ivf_scan_grid("ivfpq_scan", M, E, L, Q, P, k, seg_rows, segs, blocks);   // coati_ivf_scan's limits and grid
  if (grid < 0) return grid;
  COATI_CHECK_SHAPE(k <= coati_ivfpq_k_max(E), "ivfpq_scan: k=%d outside 1 .. %d at E=%d", k, coati_ivfpq_k_max(E), E);
  if (blocks == 0 && grid > IVFPQ_GRID_MAX) grid = IVFPQ_GRID_MAX;
  if (E <= 128)
    return ivfpq_launch<4>(codes, ids, bias, list_off, M, E, L, centres, codebook, q, Q, pair_q, pair_off, item_off, P, k, alpha, seg_rows, segs,
                           part_score, part_row, grid, s);
  return ivfpq_launch<8>(codes, ids, bias, list_off, M, E, L, centres, codebook, q, Q, pair_q, pair_off, item_off, P, k, alpha, seg_rows, segs,
                         part_score, part_row, grid, s);
}
