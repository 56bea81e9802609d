// IVF approximate search over fp8 lists (include/coati_ivf8.h): the library stored list by list as OCP e4m3 bytes (lib8 [M, E] in list
// order) with one power-of-two f32 scale per position (scale, ids, bias, list_off); a quantised query scores only the rows of the lists it
// probes.  No score is ever written to memory, no result depends on the launch geometry.  The merge (ivf_merge_kernel of ivf.hip), the
// plan (coati_ivf_plan) and the exact re-scoring of the candidates (search_rescore_kernel of search8.hip) are used as they are.
//
// ivf8_scan_kernel<TMAX>, 4 waves, one query panel of 16 pairs: ivf_scan_kernel's item loop (ivf.hip) around search8_topk_kernel's stream
// (search8.hip).  The probe table arrives inverted: the (query, list) pairs sorted by (list, query).  A work item is (list l, group of <= 16
// of its pairs, segment of seg_rows of its rows), numbered segment-major; a workgroup takes items blockIdx.x, + gridDim.x, ... and finds
// an item's list by bisection of item_off.  Per item it gathers the group's queries through pair_q into byte fragments cut as the
// library's are (columns past the group's last pair, or with a query outside 0 .. Q - 1, are zero fragments that are neither filtered nor
// stored), sets qm = alpha * qscale[query], streams positions r_begin .. r_end - 1 of the segment (stream8) and writes
// part[pair][segment][0 .. k-1] in rank order, the row being ids[position], padded with (-inf, -1).
//
// stream8 RESTATES search8_topk_kernel's stream for one panel, as radius.hip restates the bf16 one: moved into a device function that
// both kernels called, the stream cost coati_search8_topk 0.5 .. 1.2 % at E = 512 ("Quantised approximate search":
// the kernel sits at 251 of 256 VGPRs and the register allocation did not survive the move), so search8.hip stays as it is.  What must
// agree, and is pinned by tests/test_gpu_ivf8.py against the same oracles as tests/test_gpu_search8.py: a lane takes 16 CONTIGUOUS
// bytes of its row per load -- load t of lane group g is bytes 64 t + 16 g .. + 15, low 8 bytes the fragment of one
// v_mfma_f32_16x16x32_fp8_fp8 and high 8 bytes of the next, the queries cut the same way, off[t] / has[t] for E % 64 == 32; the MFMAs in
// ascending t from a zero accumulator; score = (qm * scale[row]) * acc + bias[row], then + 0.0f; the three-buffer prefetch unrolled by
// three with no load under a condition; the strict > filter; cap = k + 2 TOPK_ROWS_IT, a compaction after every iteration that left a
// count above cap - TOPK_ROWS_IT; the parity flag words.  A (query, row) pair then has the same bits in both fp8 kernels.
//  * the stream's "row" is a position of lib8 here.  Its strict > stays the tie rule: the threshold is the k-th best of positions that
//    are all SMALLER, and inside a list a smaller position is a smaller original row (the header's precondition), so an equal score
//    correctly loses;
//  * positions >= the segment's end are read at min(position, M - 1) -- inside lib8, scale and bias; they may be the next list's rows,
//    whose bytes are finite -- and dropped by the filter (position < r_end), whatever their score;
//  * every table word is clamped before it is used: p_begin <= p_end within 0 .. P, l_begin <= l_end within 0 .. M, so a position
//    streamed is in 0 .. M - 1 and a pair read in 0 .. P - 1 whatever the tables hold.
// Why every barrier is workgroup-uniform: the trip count of the item loop is item_off[L], blockIdx.x and gridDim.x; an item's list,
// pair range, row range, group and segment are computed by every thread from the same global words (item_off, pair_off, list_off) and
// the arguments, so `continue` is taken by all threads or none and the body is entered by all or none; inside stream8 the trip count
// (iters, whole) is the segment's r_begin and r_end -- the same words -- and whether to compact is read by all threads from one LDS word
// behind a barrier.  No barrier is under a lane-, wave- or column-dependent condition: a column without a query only has a zero fragment
// and stored = false.  The barrier after the write-out puts the next item's reset of the counts behind this item's reads of them.
#include <type_traits>

#include "../../include/coati_ivf8.h"
#include "topk_stream_dev.h"

// Positions [r_begin, r_end) of lib [M, E] e4m3 (both bounds workgroup-uniform; an empty range leaves empty lists) against the byte
// fragments bq[t] = bytes off[t] .. + 15 of the query in column col (zeros where the lane has no such load or the column no query),
// qm = alpha * qscale of that query, stored: the column holds a query.  On return (behind a barrier) column ql's min(k, candidates) best
// keys are sbuf[ql * cap ..] in rank order and s_cnt[ql] is their number.  sbuf [16][cap], s_cnt and s_thr [16], s_flag [2] are LDS that
// the reset below overwrites: the caller puts a barrier between its reads of the last call's lists and this call.
template <int TMAX>
__device__ __forceinline__ void stream8(const unsigned char* __restrict__ lib, const float* __restrict__ scale, long long M, int E,
                                        const float* __restrict__ bias, const uint4 (&bq)[TMAX], float qm, bool stored, const int (&off)[TMAX],
                                        long long r_begin, long long r_end, int k, int cap, topk_key_t* sbuf, int* s_cnt, float* s_thr,
                                        int* s_flag) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int r_end32 = (int)r_end;   // (< 2^31)
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;
  if (tid < 16) {
    s_cnt[tid] = 0;
    s_thr[tid] = -INFINITY;
  }
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();

  // a wave's slab of iteration it: positions r_begin + 16 (4 it + wave) .. + 15; the lane's row is slab + col.  A position >= M is read
  // at M - 1 (inside the allocation) and a result position >= r_end is dropped by the filter.  bs / ss = the bias and scale of the
  // lane's four result rows.  Every load is unconditional -- a load under a lane's or even a uniform condition makes the compiler wait
  // for the slabs in flight where the paths meet; a lane's load t at or past E (off) repeats the row's last 16 bytes against a zero
  // query fragment
  struct Slab {
    uint4 a[TMAX];
    float bs[4], ss[4];
  };
  auto load_slab = [&](Slab& d, int it) __attribute__((always_inline)) {
    const long long slab = r_begin + 16ll * (4 * min(it, iters - 1) + wave);   // (past the last iteration: its slab again, never used)
    const long long row = min(slab + col, M - 1);
    const unsigned char* src = lib + row * E;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) d.a[t] = *reinterpret_cast<const uint4*>(src + off[t]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long br = min(slab + 4 * g + r, M - 1);
      d.bs[r] = bias[br];
      d.ss[r] = scale[br];
    }
  };
  // one iteration: the slab two ahead goes into the buffer the last iteration used, then the products and the filter of `cur`
  auto step = [&](auto refills, int it, const Slab& cur, Slab& refill) __attribute__((always_inline)) {
    if constexpr (decltype(refills)::value) load_slab(refill, it + 2);
    int* const flag = s_flag + (it & 1);   // this iteration's word

    topk_f32x4 acc = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (64 * t < E) {
        const long a_lo = (long)(((unsigned long long)cur.a[t].y << 32) | cur.a[t].x);
        const long a_hi = (long)(((unsigned long long)cur.a[t].w << 32) | cur.a[t].z);
        const long b_lo = (long)(((unsigned long long)bq[t].y << 32) | bq[t].x);
        const long b_hi = (long)(((unsigned long long)bq[t].w << 32) | bq[t].z);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a_lo, b_lo, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a_hi, b_hi, acc, 0, 0, 0);
      }
    }

    // filter: the lane's four rows against its query's threshold
    const int row0 = (int)(r_begin + 16ll * (4 * it + wave)) + 4 * g;
    const float thr = s_thr[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sc = (qm * cur.ss[r]) * acc[r] + cur.bs[r];
      sc += 0.0f;   // -0 -> +0: the two must tie
      if (stored && row0 + r < r_end32 && sc > thr) {
        const int slot = atomicAdd(&s_cnt[col], 1);   // < cap: the count was <= cap - TOPK_ROWS_IT when this iteration began
        sbuf[col * cap + slot] = topk_key(sc, row0 + r);
        if (slot + 1 > cap - TOPK_ROWS_IT) *flag = 1;
      }
    }
    __syncthreads();
    const int full = *flag;   // read by every thread between two barriers with no write to it: workgroup-uniform
    if (full) {
      topk_compact<false>(sbuf, s_cnt, s_thr, 16, cap, k, wave, lane);
      __syncthreads();
      if (tid == 0) *flag = 0;   // (this word's next use is two iterations on, behind the next iteration's barrier)
    }
  };

  Slab b0, b1, b2;
#pragma unroll
  for (int t = 0; t < TMAX; ++t) b0.a[t] = b1.a[t] = b2.a[t] = make_uint4(0u, 0u, 0u, 0u);
  // Whole triples of iterations load without any condition -- the counter the compiler waits on must be right on every path, so one
  // path with fewer loads in flight would make all of them wait as if they had as few -- and the one or two iterations left over
  // run without loads: what they need is in b0 and b1.  iters, and so every condition here, is workgroup-uniform.
  const int whole = iters / 3 * 3;
  if (iters > 0) {
    load_slab(b0, 0);
    load_slab(b1, 1);
  }
  for (int it = 0; it < whole; it += 3) {
    step(std::true_type{}, it, b0, b2);
    step(std::true_type{}, it + 1, b1, b0);
    step(std::true_type{}, it + 2, b2, b1);
  }
  if (iters - whole >= 1) step(std::false_type{}, whole, b0, b2);
  if (iters - whole == 2) step(std::false_type{}, whole + 1, b1, b0);

  topk_compact<true>(sbuf, s_cnt, s_thr, 16, cap, k, wave, lane);
  __syncthreads();
}

template <int TMAX>
__global__ __launch_bounds__(256) void ivf8_scan_kernel(const unsigned char* __restrict__ lib, const float* __restrict__ scale,
                                                        const int* __restrict__ ids, const float* __restrict__ bias,
                                                        const int* __restrict__ list_off, long long M, int E, int L,
                                                        const unsigned char* __restrict__ q, const float* __restrict__ qscale, int Q,
                                                        const int* __restrict__ pair_q, const int* __restrict__ pair_off,
                                                        const int* __restrict__ item_off, long long P, int k, float alpha, int seg_rows, int segs,
                                                        int cap, float* __restrict__ part_score, int* __restrict__ part_row) {
  extern __shared__ topk_key_t sbuf[];   // [16][cap]
  __shared__ int s_cnt[16];
  __shared__ float s_thr[16];
  __shared__ int s_flag[2];
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const long long items = item_off[L];
  // which of its loads a lane has: bytes 64 t + 16 g .. + 15 of a row of E bytes (a lane-dependent answer only for the last load of an
  // E that is not a multiple of 64).  A lane without one reads the row's last 16 bytes instead (off: no branch in the stream) against
  // a zero query fragment: the library's bytes are finite e4m3 values, so those products are zeros
  bool has[TMAX];
  int off[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    has[t] = 64 * t + 16 * g < E;
    off[t] = min(64 * t + 16 * g, E - 16);
  }

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

    // the group's queries: the bytes off[t] .. + 15 of the query in column col, qm = alpha * its scale
    int qi = -1;
    if (col < nq) qi = pair_q[p0 + col];
    const bool stored = qi >= 0 && qi < Q;
    const float qm = stored ? alpha * qscale[qi] : 0.f;
    uint4 bq[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (has[t] && stored) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + off[t]);
      bq[t] = v;
    }
    stream8<TMAX>(lib, scale, M, E, bias, bq, qm, stored, off, r_begin, r_end, k, cap, sbuf, s_cnt, s_thr, s_flag);
    // (a stored position is one of r_begin .. r_end - 1 < M)
    topk_write_out(sbuf, s_cnt, cap, k, nq, (p0 * segs + sg) * k, (long long)segs * k, [&](int pos) { return ids[pos]; }, part_score, part_row);
    __syncthreads();   // the next item's reset of the counts, behind this one's reads
  }
}

int coati_ivf8_scan(const uint8_t* lib, const float* scale, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E,
                    int L, const uint8_t* q, const float* qscale, int Q, const int32_t* pair_q, const int32_t* pair_off,
                    const int32_t* item_off, int64_t P, int k, float alpha, int seg_rows, int segs, float* part_score, int32_t* part_row,
                    int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "ivf8_scan: lib8 is null");
  COATI_CHECK_ARG(scale, "ivf8_scan: scale is null");
  COATI_CHECK_ARG(ids, "ivf8_scan: ids is null");
  COATI_CHECK_ARG(bias, "ivf8_scan: bias is null");
  COATI_CHECK_ARG(list_off, "ivf8_scan: list_off is null");
  COATI_CHECK_ARG(q, "ivf8_scan: q8 is null");
  COATI_CHECK_ARG(qscale, "ivf8_scan: qscale is null");
  COATI_CHECK_ARG(pair_q, "ivf8_scan: pair_q is null");
  COATI_CHECK_ARG(pair_off, "ivf8_scan: pair_off is null");
  COATI_CHECK_ARG(item_off, "ivf8_scan: item_off is null");
  COATI_CHECK_ARG(part_score, "ivf8_scan: part_score is null");
  COATI_CHECK_ARG(part_row, "ivf8_scan: part_row is null");
  const int grid = ivf_scan_grid("ivf8_scan", M, E, L, Q, P, k, seg_rows, segs, blocks);   // coati_ivf_scan's limits and grid
  if (grid < 0) return grid;
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = (size_t)16 * cap * sizeof(topk_key_t);   // <= 32 KiB
  if (E <= 256)
    hipLaunchKernelGGL((ivf8_scan_kernel<4>), dim3(grid), dim3(256), lds, s, lib, scale, ids, bias, list_off, M, E, L, q, qscale, Q, pair_q, pair_off,
                       item_off, P, k, alpha, seg_rows, segs, cap, part_score, part_row);
  else
    hipLaunchKernelGGL((ivf8_scan_kernel<8>), dim3(grid), dim3(256), lds, s, lib, scale, ids, bias, list_off, M, E, L, q, qscale, Q, pair_q, pair_off,
                       item_off, P, k, alpha, seg_rows, segs, cap, part_score, part_row);
  COATI_LAUNCH_CHECK("ivf8_scan");
  return COATI_OK;
}
