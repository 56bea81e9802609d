// Library clustering (include/coati_cluster.h): every row's nearest centre, and the per-cluster sums of the rows.  No score matrix, no atomics;
// what is written is a function of the operands alone -- not of the grid, the stream or the run.
//
// cluster_assign_kernel, 4 waves, a workgroup takes tiles of 64 SL rows in turn (tile = blockIdx.x, + gridDim.x, ...):
//  * search_topk_kernel's arrangement: library rows are the M side of v_mfma_f32_16x16x32_bf16, centres its N side; the result map (column =
//    lane & 15, row = 4 (lane >> 4) + register) gives a lane four rows of ONE centre per panel;
//  * the roles are swapped: the wave's SL slabs of 16 rows are loaded once and stay in registers for the whole sweep (SL x E / 32 steps x
//    4 VGPRs: SL = 4 up to E = 256, SL = 2 above, at most 128 VGPRs), the centres pass through LDS in tiles of CL_TC = 32 (two panels),
//    ascending.  A B fragment read from LDS (1 KiB per wave) feeds SL MFMAs.  One instance per E / 32: with the k-steps a run-time bound
//    every step was a branch, no LDS read could move ahead of the step before it, and the sweep ran at half this rate;
//  * the LDS image of a centre tile is in fragment order, [panel][k-step][lane] 16-B slots, so that a wave's read of a fragment is one
//    contiguous KiB; two images: tile t + 1 is fetched into registers before tile t's MFMAs and written to the other image after them, one
//    barrier per tile.  The trip counts (row tiles of the workgroup, centre tiles) are workgroup-uniform: no barrier is under a lane- or
//    wave-dependent condition;
//  * a lane keeps a running (score, centre) for each of its 4 SL result rows.  It meets its own centres in ascending order and replaces on
//    `>`, strictly, so the lower index keeps a tie.  A column >= K of the last tile is read from centre K - 1 (inside the allocation) and
//    scores -inf, which never passes the `>`: it cannot win whatever the scores' signs;
//  * the 16 lanes of a row meet once after the sweep (4 xor steps), on (score, then lower index): a lane that saw no centre at all (K < 16)
//    holds (-inf, INT_MAX) and loses to any real one;
//  * rows >= N of the last tile are read at row N - 1 and never stored.
//
// cluster_partial_kernel / cluster_finish_kernel: the per-destination sum pass over an inverted index.  The rows of every cluster (order,
// offsets) are cut into chunks of CL_CH; work item i = chunk i - item_off[k] of the cluster k found by bisection in item_off.  A workgroup
// takes items in turn; E / 8 threads span a row (16-B loads), the 256 / (E / 8) groups of them take the chunk's rows p, p + R, ... in order,
// and the groups' f32 sums are added in group order through LDS into part[item].  The finish adds a cluster's partial rows in chunk order.
#include "../../include/coati_cluster.h"
#include "kernels.h"

#define CL_E_MAX 512
#define CL_K_MAX 4096
#define CL_TC 32     // centres per LDS tile
#define CL_CH 512    // rows per work item of the sums

typedef float cluster_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cluster_u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of bf16

// A thread's 16-B pieces of centre tile t: piece i = (k-step s = i / 128, centre (i / 4) % 32, quarter g' = i % 4 of the step's 64 bytes)
// -> slot [panel][s][16 g' + column] of the LDS image.  Four lanes read 64 contiguous bytes; a wave's 64 pieces are the 64 slots of one
// fragment.  (The staging registers are a native 16-byte vector type: as an array of HIP's uint4 structs they stayed in scratch memory.)
template <int KS, int NST>
__device__ __forceinline__ void cluster_fetch(cluster_u32x4 (&st)[NST], const bf16_t* __restrict__ c, int K, int t, int tid) {
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    const int i = min(tid + 256 * j, CL_TC * KS * 4 - 1);   // (an odd KS: the last round's upper half loads a piece it never stores)
    const int cc = min(t * CL_TC + ((i >> 2) & (CL_TC - 1)), K - 1);
    st[j] = *reinterpret_cast<const cluster_u32x4*>(c + (long long)cc * (32 * KS) + 32 * (i >> 7) + 8 * (i & 3));
  }
}
template <int KS, int NST>
__device__ __forceinline__ void cluster_stash(const cluster_u32x4 (&st)[NST], cluster_u32x4* image, int tid) {
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    const int i = tid + 256 * j;
    if (256 * j + 255 < CL_TC * KS * 4 || i < CL_TC * KS * 4) {
      const int cc = (i >> 2) & (CL_TC - 1);
      image[(((cc >> 4) * KS + (i >> 7)) << 6) + ((i & 3) << 4) + (cc & 15)] = st[j];
    }
  }
}

template <int KS, int SL>
__global__ __launch_bounds__(256, 2) void cluster_assign_kernel(const bf16_t* __restrict__ lib, long long N, const float* __restrict__ row_bias,
                                                                const bf16_t* __restrict__ c, int K, const float* __restrict__ cbias,
                                                                int* __restrict__ assign, float* __restrict__ best) {
  extern __shared__ cluster_u32x4 cl_tile[];   // [2][2 panels][KS][64 lanes]
  constexpr int ROWS = 64 * SL, E = 32 * KS;   // (KS a template argument: the sweep is straight-line code, its LDS reads ahead of its MFMAs)
  constexpr int img = 2 * KS * 64;             // 16-B slots of one image
  constexpr int pieces = CL_TC * KS * 4;       // 16-B pieces of a centre tile
  constexpr int NST = (pieces + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ctiles = (K + CL_TC - 1) / CL_TC;
  const long long rtiles = (N + ROWS - 1) / ROWS;

  cluster_u32x4 st[NST];

  for (long long rt = blockIdx.x; rt < rtiles; rt += gridDim.x) {
    // the wave's slabs: rows r0 + 16 sl + (0 .. 15); A[row = col][k = 32 s + 8 g + j]
    const long long r0 = rt * ROWS + (long long)wave * 16 * SL;
    cluster_u32x4 a[SL][KS];
#pragma unroll
    for (int sl = 0; sl < SL; ++sl) {
      const long long row = min(r0 + 16 * sl + col, N - 1);
      const cluster_u32x4* src = reinterpret_cast<const cluster_u32x4*>(lib + row * E + 8 * g);
#pragma unroll
      for (int s = 0; s < KS; ++s) a[sl][s] = src[4 * s];
    }
    float bs[SL][4];
    int bi[SL][4];
#pragma unroll
    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bs[sl][r] = -INFINITY;
        bi[sl][r] = 0x7fffffff;
      }

    cluster_fetch<KS, NST>(st, c, K, 0, tid);
    cluster_stash<KS, NST>(st, cl_tile, tid);
    __syncthreads();
    for (int t = 0; t < ctiles; ++t) {
      if (t + 1 < ctiles) cluster_fetch<KS, NST>(st, c, K, t + 1, tid);
      const cluster_u32x4* tile = cl_tile + (t & 1) * img;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int ci = t * CL_TC + 16 * p + col;
        const float cb = ci < K ? (cbias ? cbias[ci] : 0.f) : -INFINITY;   // a padded column scores -inf: it never passes the strict >
        cluster_f32x4 acc[SL];
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) acc[sl] = cluster_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const bf16x8 b = __builtin_bit_cast(bf16x8, tile[((p * KS + s) << 6) + lane]);
#pragma unroll
          for (int sl = 0; sl < SL; ++sl)
            acc[sl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[sl][s]), b, acc[sl], 0, 0, 0);
        }
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sc = acc[sl][r] + cb;
            if (sc > bs[sl][r]) {
              bs[sl][r] = sc;
              bi[sl][r] = ci;
            }
          }
      }
      if (t + 1 < ctiles) cluster_stash<KS, NST>(st, cl_tile + ((t + 1) & 1) * img, tid);   // (that image's readers were tile t - 1's, behind the barrier that ended it)
      __syncthreads();
    }

    // the 16 lanes of a row: the larger score, the lower centre among equal ones
#pragma unroll
    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = bs[sl][r];
        int i = bi[sl][r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          const float so = __shfl_xor(s, m, 64);
          const int io = __shfl_xor(i, m, 64);
          if (so > s || (so == s && io < i)) {
            s = so;
            i = io;
          }
        }
        const long long row = r0 + 16 * sl + 4 * g + r;
        if (col == 4 * (sl & 3) + r && row < N) {
          const bool out = row_bias && row_bias[row] == -INFINITY;
          assign[row] = out ? -1 : i;
          best[row] = out ? -INFINITY : s + 0.0f;   // -0 -> +0 (the comparisons above take the two for equal anyway)
        }
      }
  }
}

// part[item, :] = the sum of the item's rows.  LPR = E / 8 threads per row, R = 256 / LPR groups; group p adds rows p, p + R, ... of the chunk
// in that order, then the groups' sums are added in group order.
__global__ __launch_bounds__(256) void cluster_partial_kernel(const bf16_t* __restrict__ lib, long long N, int E, const int* __restrict__ order,
                                                              long long M, const int* __restrict__ offsets, const int* __restrict__ item_off,
                                                              int K, float* __restrict__ part, long long items_max) {
  __shared__ float red[2048];   // [R][E], R * E <= 256 * 8
  const int tid = threadIdx.x;
  const int lpr = E >> 3, R = 256 / lpr;
  const int p = tid / lpr, pc = tid - p * lpr;
  const long long items = min((long long)item_off[K], items_max);
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int lo = item_owner(item_off, K, it);   // the cluster of item `it`
    const long long beg = max(0ll, (long long)offsets[lo] + (it - item_off[lo]) * CL_CH);
    const long long end = min(min((long long)offsets[lo + 1], beg + CL_CH), M);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (p < R) {
#pragma unroll 4
      for (long long i = beg + p; i < end; i += R) {
        const long long row = order[i];
        const long long rr = row >= 0 && row < N ? row : 0;
        const uint4 v = *reinterpret_cast<const uint4*>(lib + rr * E + 8 * pc);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[2 * j] += __uint_as_float(w[j] << 16);
          acc[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) red[p * E + 8 * pc + j] = acc[j];
    }
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
      float s = red[e];
      for (int q = 1; q < R; ++q) s += red[q * E + e];
      part[it * E + e] = s;
    }
    __syncthreads();
  }
}

// sums[k, :] = the cluster's partial rows added in chunk order; zeros for none
__global__ __launch_bounds__(256) void cluster_finish_kernel(const float* __restrict__ part, const int* __restrict__ item_off, int E,
                                                             long long items_max, float* __restrict__ sums) {
  const int k = blockIdx.x;
  const long long lo = max(0ll, (long long)item_off[k]), hi = min((long long)item_off[k + 1], items_max);
  for (int e = threadIdx.x; e < E; e += 256) {
    float s = 0.f;
    for (long long i = lo; i < hi; ++i) s += part[i * E + e];
    sums[(long long)k * E + e] = s;
  }
}

static int cluster_check(const char* what, long long N, int E, int K, int blocks) {
  COATI_CHECK_SHAPE(E >= 32 && E <= CL_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, CL_E_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "%s: N=%lld outside 1 .. 2^31 - 1", what, N);
  COATI_CHECK_SHAPE(K >= 1 && K <= CL_K_MAX, "%s: K=%d outside 1 .. %d", what, K, CL_K_MAX);
  COATI_CHECK_SHAPE(blocks >= 0, "%s: blocks=%d < 0", what, blocks);
  return COATI_OK;
}

template <int KS, int SL>
static int cluster_assign_launch(const bf16_t* lib, long long N, const float* row_bias, const bf16_t* c, int K, const float* cbias,
                                 int* assign, float* best, int blocks, hipStream_t s) {
  const long long rtiles = (N + 64 * SL - 1) / (64 * SL);
  const int grid = (int)(blocks > 0 && blocks < rtiles ? blocks : rtiles);
  const size_t lds = (size_t)2 * 2 * KS * 64 * sizeof(cluster_u32x4);   // <= 64 KiB at E = 512
  hipLaunchKernelGGL((cluster_assign_kernel<KS, SL>), dim3(grid), dim3(256), lds, s, lib, N, row_bias, c, K, cbias, assign, best);
  COATI_LAUNCH_CHECK("cluster_assign");
  return COATI_OK;
}

int coati_cluster_assign(const uint16_t* lib, int64_t N, int E, const float* row_bias, const uint16_t* c, int K, const float* cbias,
                         int32_t* assign, float* best, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "cluster_assign: lib is null");
  COATI_CHECK_ARG(c, "cluster_assign: c is null");
  COATI_CHECK_ARG(assign, "cluster_assign: assign is null");
  COATI_CHECK_ARG(best, "cluster_assign: best is null");
  COATI_TRY(cluster_check("cluster_assign", N, E, K, blocks));
  switch (E >> 5) {
#define CL_CASE(KS) \
  case KS: return cluster_assign_launch<KS, (KS <= 8 ? 4 : 2)>(lib, N, row_bias, c, K, cbias, assign, best, blocks, s);
    CL_CASE(1) CL_CASE(2) CL_CASE(3) CL_CASE(4) CL_CASE(5) CL_CASE(6) CL_CASE(7) CL_CASE(8)
    CL_CASE(9) CL_CASE(10) CL_CASE(11) CL_CASE(12) CL_CASE(13) CL_CASE(14) CL_CASE(15) CL_CASE(16)
#undef CL_CASE
  }
  coati_set_error("cluster_assign: E=%d has no kernel", E);
  return COATI_ESHAPE;
}

int coati_cluster_chunk(void) { return CL_CH; }

int64_t coati_cluster_items_max(int64_t M, int K) {
  if (!(M >= 0 && M < (1ll << 31) && K >= 1 && K <= CL_K_MAX)) {
    coati_set_error("cluster_items_max: M=%lld K=%d out of range", (long long)M, K);
    return COATI_ESHAPE;
  }
  return M / CL_CH + K;
}

int coati_cluster_sums(const uint16_t* lib, int64_t N, int E, const int32_t* order, int64_t M, const int32_t* offsets,
                       const int32_t* item_off, int K, float* part, int64_t items_max, float* sums, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "cluster_sums: lib is null");
  COATI_CHECK_ARG(order, "cluster_sums: order is null");
  COATI_CHECK_ARG(offsets, "cluster_sums: offsets is null");
  COATI_CHECK_ARG(item_off, "cluster_sums: item_off is null");
  COATI_CHECK_ARG(part, "cluster_sums: part is null");
  COATI_CHECK_ARG(sums, "cluster_sums: sums is null");
  COATI_TRY(cluster_check("cluster_sums", N, E, K, blocks));
  COATI_CHECK_SHAPE(M >= 1 && M <= N, "cluster_sums: M=%lld outside 1 .. N=%lld", (long long)M, (long long)N);
  COATI_CHECK_SHAPE(items_max >= M / CL_CH + K, "cluster_sums: items_max=%lld < M / %d + K = %lld", (long long)items_max, CL_CH, (long long)M / CL_CH + K);
  const long long most = M / CL_CH + K;
  const int grid = (int)(blocks > 0 && blocks < most ? blocks : (most < 4096 ? most : 4096));
  hipLaunchKernelGGL(cluster_partial_kernel, dim3(grid), dim3(256), 0, s, lib, N, E, order, M, offsets, item_off, K, part, items_max);
  COATI_LAUNCH_CHECK("cluster_partial");
  hipLaunchKernelGGL(cluster_finish_kernel, dim3(K), dim3(256), 0, s, part, item_off, E, items_max, sums);
  COATI_LAUNCH_CHECK("cluster_finish");
  return COATI_OK;
}
