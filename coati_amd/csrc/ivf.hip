// IVF approximate search (include/coati_ivf.h): the library is stored list by list (lib [M, E] bf16 in list order, ids, bias, list_off), a
// query scores only the rows of the lists it probes.  No score is ever written to memory, no result depends on the launch geometry.
//
// ivf_scan_kernel, 4 waves.  The probe table arrives inverted: the (query, list) pairs sorted by (list, query).  A work item is (list l,
// group of <= 16 of its pairs, segment of seg_rows of its rows); a workgroup takes items blockIdx.x, + gridDim.x, ... and finds an item's
// list by bisection of item_off, so the grid is sized without the host knowing the item count.  Items are numbered segment-major: items
// i, i + 1 share the row segment and differ in the pair group, so a segment brought in for one group is found in the caches by the next.
// Per item a workgroup gathers the group's queries through pair_q into B fragments (columns past the group's last pair, or with a query
// outside 0 .. Q - 1, are zero fragments that are neither filtered nor stored), runs topk_stream<KSMAX, 1> (topk_stream_dev.h: the exact
// search's body, so a (query, row) score has the same bits in both kernels) over the segment's positions, and writes
// part[pair][segment][0 .. k-1] in rank order, the row being ids[position], padded with (-inf, -1).
//  * the body's "row" is a position of lib here.  Its strict > stays the tie rule: the threshold is the k-th best of positions that are
//    all SMALLER, and inside a list a smaller position is a smaller original row (the header's precondition), so an equal score correctly
//    loses;
//  * every trip count -- items of the workgroup, iterations of the item -- is computed by every thread from the same global words:
//    workgroup-uniform.  No barrier is under a lane-, wave- or item-dependent condition (an item that is skipped is skipped whole, by
//    every thread, before the body is entered).
// Positions >= the segment's end are read from a clamped address (inside lib) and masked to -inf after the MFMA.
//
// ivf_merge_kernel, one workgroup per query: its partial lists (through pair_slot; of entry j only the segments its list really has, from
// list_off -- a slot no item wrote is never read) become 64-bit keys (score key << 32 | ~row) in LDS, unique over the query since a row
// lives in one list.  An 8-pass radix select finds the k-th largest key, the <= k survivors are ranked by counting.  Key descending is
// score descending, original row ascending among equal scores.
#include "../../include/coati_ivf.h"
#include "search_host.h"

#define IVF_E_MAX 512
#define IVF_L_MAX 4096
#define IVF_NPROBE_MAX 128
#define IVF_MERGE_MAX 16384    // nprobe * segs * k: the merge's row of 64-bit keys in 128 KiB of LDS
#define IVF_SEG_MIN 128        // rows of the shortest segment coati_ivf_plan proposes
#define IVF_GRID_MAX 2048

template <int KSMAX>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const bf16_t* __restrict__ lib, const int* __restrict__ ids, const float* __restrict__ bias,
                                                       const int* __restrict__ list_off, long long M, int E, int L, const bf16_t* __restrict__ q,
                                                       int Q, const int* __restrict__ pair_q, const int* __restrict__ pair_off,
                                                       const int* __restrict__ item_off, long long P, int k, float alpha, int seg_rows, int segs,
                                                       int cap, float* __restrict__ part_score, int* __restrict__ part_row) {
  extern __shared__ topk_key_t sbuf[];   // [16][cap]
  __shared__ int s_cnt[16];
  __shared__ float s_thr[16];
  __shared__ int s_flag[2];
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
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

    // the group's queries: B[k = 32 s + 8 g + j][column = col]
    int qi = -1;
    if (col < nq) qi = pair_q[p0 + col];
    const bool stored[1] = {qi >= 0 && qi < Q};
    bf16x8 bq[1][KSMAX];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored[0]) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[0][s] = __builtin_bit_cast(bf16x8, v);
    }
    topk_stream<KSMAX, 1>(lib, M, E, bias, bq, 1, stored, r_begin, r_end, alpha, k, cap, sbuf, s_cnt, s_thr, s_flag);
    // (a stored position is one of r_begin .. r_end - 1 < M)
    topk_write_out(sbuf, s_cnt, cap, k, nq, (p0 * segs + sg) * k, (long long)segs * k, [&](int pos) { return ids[pos]; }, part_score, part_row);
    __syncthreads();   // the next item's reset of the counts, behind this one's reads
  }
}

__global__ __launch_bounds__(256) void ivf_merge_kernel(const float* __restrict__ part_score, const int* __restrict__ part_row,
                                                        const int* __restrict__ probes, const int* __restrict__ pair_slot, long long P,
                                                        const int* __restrict__ list_off, int L, int nprobe, int k, int seg_rows, int segs,
                                                        float* __restrict__ out_score, long long* __restrict__ out_row) {
  extern __shared__ topk_key_t mkeys[];   // [nprobe * segs * k]
  __shared__ int hist[256];
  __shared__ topk_key_t s_prefix;
  __shared__ int s_need, s_n;
  __shared__ topk_key_t top[TOPK_MAX];
  __shared__ long long s_slot[IVF_NPROBE_MAX];
  __shared__ int s_nseg[IVF_NPROBE_MAX];
  const int tid = threadIdx.x;
  const long long qi = blockIdx.x;
  if (tid < nprobe) {
    const int l = probes[qi * nprobe + tid];
    const long long slot = pair_slot[qi * nprobe + tid];
    int nseg = 0;
    if (l >= 0 && l < L && slot >= 0 && slot < P) {
      const long long rows = (long long)list_off[l + 1] - list_off[l];
      if (rows > 0) nseg = (int)min((rows + seg_rows - 1) / seg_rows, (long long)segs);
    }
    s_slot[tid] = slot;
    s_nseg[tid] = nseg;
  }
  if (tid == 0) {
    s_prefix = 0ull;
    s_need = k;
    s_n = 0;
  }
  __syncthreads();
  // the query's candidates; what is padding, or a slot the scan did not write, is key 0 -- below every real key
  const int sk = segs * k, V = nprobe * sk;
  for (int i = tid; i < V; i += 256) {
    const int j = i / sk, rem = i - j * sk, sg = rem / k;
    topk_key_t key = 0ull;
    if (sg < s_nseg[j]) {
      const long long o = s_slot[j] * sk + rem;
      const float sc = part_score[o];
      const int row = part_row[o];
      if (row >= 0 && sc > -INFINITY) key = topk_key(sc, row);
    }
    mkeys[i] = key;
  }
  __syncthreads();
  // radix select of the k-th largest key (V >= k): after pass p the top 8 (p + 1) bits of it are known
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    const topk_key_t mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    hist[tid] = 0;
    __syncthreads();
    const topk_key_t prefix = s_prefix;
    for (int i = tid; i < V; i += 256) {
      const topk_key_t key = mkeys[i];
      if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int need = s_need, bin = 255;
      for (; bin > 0; --bin) {
        if (hist[bin] >= need) break;
        need -= hist[bin];
      }
      s_need = need;
      s_prefix = prefix | ((topk_key_t)bin << shift);
    }
    __syncthreads();
  }
  // survivors: the real keys >= the k-th largest.  Real keys are unique, so there are at most k (the bound check only guards a caller that
  // named a list twice)
  const topk_key_t tau = s_prefix;
  for (int i = tid; i < V; i += 256) {
    const topk_key_t key = mkeys[i];
    if (key != 0ull && key >= tau) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < TOPK_MAX) top[slot] = key;
    }
  }
  __syncthreads();
  const int n = min(min(s_n, k), TOPK_MAX);
  if (tid < k) {
    if (tid < n) {
      const topk_key_t mine = top[tid];
      int rank = 0;
      for (int j2 = 0; j2 < n; ++j2) rank += top[j2] > mine ? 1 : 0;
      out_score[qi * k + rank] = key2f((unsigned)(mine >> 32));
      out_row[qi * k + rank] = (long long)(int)~(unsigned)mine;
    } else {
      out_score[qi * k + tid] = -INFINITY;
      out_row[qi * k + tid] = -1;
    }
  }
}

static int ivf_check_common(const char* what, int L, int Q, int k, int seg_rows, int segs) {
  COATI_CHECK_SHAPE(L >= 1 && L <= IVF_L_MAX, "%s: L=%d outside 1 .. %d", what, L, IVF_L_MAX);
  COATI_CHECK_SHAPE(Q >= 1, "%s: Q=%d < 1", what, Q);
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX, "%s: k=%d outside 1 .. %d", what, k, TOPK_MAX);
  COATI_CHECK_SHAPE(seg_rows >= TOPK_ROWS_IT && seg_rows % TOPK_ROWS_IT == 0, "%s: seg_rows=%d is not a positive multiple of %d", what, seg_rows,
                    TOPK_ROWS_IT);
  COATI_CHECK_SHAPE(segs >= 1, "%s: segs=%d < 1", what, segs);
  return COATI_OK;
}

// The checks and the grid that the scan shares with its fp8 form (ivf8.hip): the limits of coati_ivf_scan's contract, then
// min(blocks or IVF_GRID_MAX, the most items P pairs can make) workgroups.  Returns the grid (>= 1) or a negative code.
int ivf_scan_grid(const char* what, long long M, int E, int L, int Q, long long P, int k, int seg_rows, int segs, int blocks) {
  COATI_CHECK_SHAPE(E >= 32 && E <= IVF_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, IVF_E_MAX);
  COATI_CHECK_SHAPE(M >= 1 && M < (1ll << 31), "%s: M=%lld outside 1 .. 2^31 - 1", what, M);
  COATI_CHECK_SHAPE(P >= 1 && P < (1ll << 31), "%s: P=%lld outside 1 .. 2^31 - 1", what, P);
  COATI_TRY(ivf_check_common(what, L, Q, k, seg_rows, segs));
  COATI_CHECK_SHAPE(blocks >= 0, "%s: blocks=%d < 0", what, blocks);
  // the most items P pairs can make: every list with pairs has at most pairs_l / 16 + 1 groups, each of at most segs segments
  const long long lists = P < L ? P : L, most = (P / 16 + lists) * segs;
  return (int)(blocks > 0 ? (blocks < most ? blocks : most) : (most < IVF_GRID_MAX ? most : IVF_GRID_MAX));
}

int coati_ivf_scan(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                   const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P, int k,
                   float alpha, int seg_rows, int segs, float* part_score, int32_t* part_row, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "ivf_scan: lib is null");
  COATI_CHECK_ARG(ids, "ivf_scan: ids is null");
  COATI_CHECK_ARG(list_off, "ivf_scan: list_off is null");
  COATI_CHECK_ARG(q, "ivf_scan: q is null");
  COATI_CHECK_ARG(pair_q, "ivf_scan: pair_q is null");
  COATI_CHECK_ARG(pair_off, "ivf_scan: pair_off is null");
  COATI_CHECK_ARG(item_off, "ivf_scan: item_off is null");
  COATI_CHECK_ARG(part_score, "ivf_scan: part_score is null");
  COATI_CHECK_ARG(part_row, "ivf_scan: part_row is null");
  const int grid = ivf_scan_grid("ivf_scan", M, E, L, Q, P, k, seg_rows, segs, blocks);
  if (grid < 0) return grid;
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = (size_t)16 * cap * sizeof(topk_key_t);   // <= 32 KiB
  if (E <= 256)
    hipLaunchKernelGGL((ivf_scan_kernel<8>), dim3(grid), dim3(256), lds, s, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P,
                       k, alpha, seg_rows, segs, cap, part_score, part_row);
  else
    hipLaunchKernelGGL((ivf_scan_kernel<16>), dim3(grid), dim3(256), lds, s, lib, ids, bias, list_off, M, E, L, q, Q, pair_q, pair_off, item_off, P,
                       k, alpha, seg_rows, segs, cap, part_score, part_row);
  COATI_LAUNCH_CHECK("ivf_scan");
  return COATI_OK;
}

int coati_ivf_merge(const float* part_score, const int32_t* part_row, const int32_t* probes, const int32_t* pair_slot, int64_t P,
                    const int32_t* list_off, int L, int Q, int nprobe, int k, int seg_rows, int segs, float* out_score, int64_t* out_row,
                    void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(part_score, "ivf_merge: part_score is null");
  COATI_CHECK_ARG(part_row, "ivf_merge: part_row is null");
  COATI_CHECK_ARG(probes, "ivf_merge: probes is null");
  COATI_CHECK_ARG(pair_slot, "ivf_merge: pair_slot is null");
  COATI_CHECK_ARG(list_off, "ivf_merge: list_off is null");
  COATI_CHECK_ARG(out_score, "ivf_merge: out_score is null");
  COATI_CHECK_ARG(out_row, "ivf_merge: out_row is null");
  COATI_CHECK_SHAPE(P >= 1 && P < (1ll << 31), "ivf_merge: P=%lld outside 1 .. 2^31 - 1", (long long)P);
  COATI_TRY(ivf_check_common("ivf_merge", L, Q, k, seg_rows, segs));
  COATI_CHECK_SHAPE(nprobe >= 1 && nprobe <= IVF_NPROBE_MAX, "ivf_merge: nprobe=%d outside 1 .. %d", nprobe, IVF_NPROBE_MAX);
  COATI_CHECK_SHAPE((long long)nprobe * segs * k <= IVF_MERGE_MAX, "ivf_merge: nprobe=%d lists of segs=%d segments of k=%d exceed nprobe * segs * k <= %d",
                    nprobe, segs, k, IVF_MERGE_MAX);
  COATI_TRY(max_dynamic_lds<ivf_merge_kernel>("ivf_merge", IVF_MERGE_MAX * (int)sizeof(topk_key_t)));
  hipLaunchKernelGGL(ivf_merge_kernel, dim3(Q), dim3(256), (size_t)nprobe * segs * k * sizeof(topk_key_t), s, part_score, part_row, probes,
                     pair_slot, P, list_off, L, nprobe, k, seg_rows, segs, out_score, LL(out_row));
  COATI_LAUNCH_CHECK("ivf_merge");
  return COATI_OK;
}

// The seg_rows coati_ivf_scan is given by default: Q * nprobe pairs (at small Q every pair is a group of its own) times the segments of a
// list should fill the device; no segment below IVF_SEG_MIN rows; nprobe * segs * k within the merge's row.  Host arithmetic only.
int64_t coati_ivf_plan(int64_t max_list_rows, int Q, int nprobe, int k) {
  COATI_CHECK_SHAPE(max_list_rows >= 1 && max_list_rows < (1ll << 31), "ivf_plan: max_list_rows=%lld outside 1 .. 2^31 - 1", (long long)max_list_rows);
  COATI_CHECK_SHAPE(Q >= 1, "ivf_plan: Q=%d < 1", Q);
  COATI_CHECK_SHAPE(nprobe >= 1 && nprobe <= IVF_NPROBE_MAX, "ivf_plan: nprobe=%d outside 1 .. %d", nprobe, IVF_NPROBE_MAX);
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX, "ivf_plan: k=%d outside 1 .. %d", k, TOPK_MAX);
  const long long by_merge = IVF_MERGE_MAX / ((long long)nprobe * k);
  COATI_CHECK_SHAPE(by_merge >= 1, "ivf_plan: nprobe=%d times k=%d exceeds nprobe * segs * k <= %d", nprobe, k, IVF_MERGE_MAX);
  const long long pairs = (long long)Q * nprobe;
  long long segs = (TOPK_DEVICE_SLOTS + pairs - 1) / pairs;
  segs = segs < by_merge ? segs : by_merge;
  long long seg_rows = ((max_list_rows + segs - 1) / segs + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT * TOPK_ROWS_IT;
  seg_rows = seg_rows > IVF_SEG_MIN ? seg_rows : IVF_SEG_MIN;
  COATI_CHECK_SHAPE(seg_rows < (1ll << 31), "ivf_plan: max_list_rows=%lld in %lld segments: no multiple of %d below 2^31 holds a segment",
                    (long long)max_list_rows, segs, TOPK_ROWS_IT);
  return seg_rows;
}
