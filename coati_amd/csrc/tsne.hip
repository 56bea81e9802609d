// Embedding maps (include/coati_tsne.h): exact t-SNE in two dimensions.  Everything is f32 on the vector ALU, no MFMA, no atomics; what is
// written is a function of the operands alone -- not of the grid, of a workspace, the stream or the run.
//
// tsne_affinities_kernel: one wave per row of the kNN graph (k <= 128: two entries a lane).  The bisection on beta runs `steps` times with
// no early exit; the row's sums are wave butterflies (xor 32 .. 1), which leave the SAME bits in every lane -- a + b and b + a are one
// value -- so the 64 lanes take the same branch without a broadcast.
//
// tsne_repulsion_kernel: the all-pairs term.  A workgroup owns a tile of TS_TI = 512 points (two per thread: one LDS read feeds both) and
// sweeps the points j in chunks of TS_J = 1024 through LDS; every lane reads the same y_j, a broadcast read.  Per pair: 2 sub, 2 fma for
// 1 + |d|^2, v_rcp_f32 (1 ulp; d >= 1, no denormal operand), 1 mul, 2 fma, 1 add -- 9 instructions, one of them transcendental (issue cost
// 8 cycles against 4: DESIGN.md section 6).  Every operation is written as the instruction it is (fmaf, or a lone sub / mul / add that
// has nothing to contract with), because the loop exists twice: only the chunk that holds the lane's own point pays the j != i compare,
// and both forms must leave the same bits.  The own point adds +0 to z, and its force is an exact zero anyway.
// The order of the additions is fixed by TS_J alone: a chunk's partial from zero in ascending j, the partials in ascending chunk order.
// With few tiles (N small) the (tile, chunk) pairs are spread over the grid, the partials go through `part` [chunk][3][N] and
// tsne_repulsion_finish_kernel adds them in that order -- the same additions.
//
// tsne_step_kernel: one wave per row of the CSR joint P.  Lane l takes the row's entries l, l + 64, ... in order, the 64 sums meet in the
// butterfly, lane 0 forms the gradient and sklearn's gains / momentum update for the row's two coordinates.
#include <float.h>

#include "../../include/coati_tsne.h"
#include "kernels.h"

#define TS_J 1024          // points per chunk of the repulsion (the summation order hangs on it)
#define TS_R 2             // points per thread
#define TS_TI (256 * TS_R) // points per workgroup tile
#define TS_SPLIT_BELOW 1024   // tiles: with fewer, and a workspace, the chunks are work items of their own
#define TS_K_MAX 128

__device__ __forceinline__ float tsne_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void tsne_affinities_kernel(const float* __restrict__ d2, const int* __restrict__ nbr, long long N, int k,
                                                              float log_perp, int steps, float* __restrict__ p, float* __restrict__ beta) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;   // (no barrier below)
  const float* dr = d2 + i * k;
  const int* nr = nbr + i * k;
  const bool v0 = lane < k && nr[lane] >= 0, v1 = lane + 64 < k && nr[lane + 64] >= 0;
  float a0 = v0 ? dr[lane] : INFINITY, a1 = v1 ? dr[lane + 64] : INFINITY;
  const float dmin = tsne_wave_min(fminf(a0, a1));
  if (dmin == INFINITY) {   // no valid entry (or none finite): zeros
    if (lane < k) p[i * k + lane] = 0.f;
    if (lane + 64 < k) p[i * k + lane + 64] = 0.f;
    if (beta && lane == 0) beta[i] = 0.f;
    return;
  }
  a0 = v0 ? a0 - dmin : 0.f;
  a1 = v1 ? a1 - dmin : 0.f;
  float b = 1.f, lo = 0.f, hi = INFINITY;
  for (int s = 0; s < steps; ++s) {
    const float p0 = v0 ? expf(-b * a0) : 0.f, p1 = v1 ? expf(-b * a1) : 0.f;
    const float S = wave_sum(p0 + p1);                 // >= 1: the nearest entry has d = 0
    const float T = wave_sum(p0 * a0 + p1 * a1);       // (p = 0 where b d overflowed: 0 times a finite d)
    const float H = logf(S) + b * T / S;
    if (H > log_perp) {
      lo = b;
      b = hi == INFINITY ? fminf(2.f * b, FLT_MAX) : 0.5f * (b + hi);   // (never inf: inf times d = 0 would be NaN)
    } else {
      hi = b;
      b = 0.5f * (b + lo);
    }
  }
  const float p0 = v0 ? expf(-b * a0) : 0.f, p1 = v1 ? expf(-b * a1) : 0.f;
  const float S = wave_sum(p0 + p1);
  if (lane < k) p[i * k + lane] = p0 / S;
  if (lane + 64 < k) p[i * k + lane + 64] = p1 / S;
  if (beta && lane == 0) beta[i] = b;
}

// One chunk's partial sums for the thread's TS_R points, from zero, in ascending j.  SELF: the chunk holds one of the thread's own points
// (at tile offset si[r], else -1), which adds +0 to z in place of its q = 1
template <bool SELF>
__device__ __forceinline__ void tsne_chunk_sum(const float2* tile, int cnt, const float (&xi)[TS_R], const float (&yi)[TS_R], const int (&si)[TS_R],
                                               float (&px)[TS_R], float (&py)[TS_R], float (&pz)[TS_R]) {
#pragma unroll 4
  for (int t = 0; t < cnt; ++t) {
    const float2 yj = tile[t];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
      const float dx = xi[r] - yj.x, dy = yi[r] - yj.y;
      const float d = fmaf(dx, dx, fmaf(dy, dy, 1.f));
      const float q = __builtin_amdgcn_rcpf(d);
      const float q2 = q * q;
      px[r] = fmaf(q2, dx, px[r]);
      py[r] = fmaf(q2, dy, py[r]);
      pz[r] = pz[r] + (SELF && t == si[r] ? 0.f : q);
    }
  }
}

// items: SPLIT ? tiles * nchunks (item = tile * nchunks + chunk, the partial written to part [nchunks][3][N]) : tiles (all chunks, rep / z written)
template <bool SPLIT>
__global__ __launch_bounds__(256) void tsne_repulsion_kernel(const float2* __restrict__ y, long long N, float* __restrict__ rep, float* __restrict__ z,
                                                             float* __restrict__ part, int nchunks, long long items) {
  __shared__ float2 tile[TS_J];
  const int tid = threadIdx.x;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {   // (workgroup-uniform trip counts: the barriers below are met by all)
    const long long it = SPLIT ? item / nchunks : item;
    const int c0 = SPLIT ? (int)(item - it * nchunks) : 0, c1 = SPLIT ? c0 + 1 : nchunks;
    long long ii[TS_R];
    float xi[TS_R], yi[TS_R], tx[TS_R], ty[TS_R], tz[TS_R];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
      ii[r] = it * TS_TI + tid + 256 * r;
      const float2 v = y[ii[r] < N ? ii[r] : N - 1];   // a point past the end repeats the last one and is never stored
      xi[r] = v.x, yi[r] = v.y;
      tx[r] = ty[r] = tz[r] = 0.f;
    }
    for (int c = c0; c < c1; ++c) {
      const long long j0 = (long long)c * TS_J;
      const int cnt = (int)(N - j0 < TS_J ? N - j0 : TS_J);
      __syncthreads();   // the readers of the chunk before
      for (int t = tid; t < cnt; t += 256) tile[t] = y[j0 + t];
      __syncthreads();
      int si[TS_R];
      float px[TS_R], py[TS_R], pz[TS_R];
      bool self = false;
#pragma unroll
      for (int r = 0; r < TS_R; ++r) {
        const bool own = ii[r] >= j0 && ii[r] < j0 + cnt;
        si[r] = own ? (int)(ii[r] - j0) : -1;
        self |= own;
        px[r] = py[r] = pz[r] = 0.f;
      }
      // (TS_TI, 256 and TS_J are multiples of 64: a wave's points lie in one chunk, the branch does not diverge)
      if (self) tsne_chunk_sum<true>(tile, cnt, xi, yi, si, px, py, pz);
      else tsne_chunk_sum<false>(tile, cnt, xi, yi, si, px, py, pz);
#pragma unroll
      for (int r = 0; r < TS_R; ++r) {
        if (SPLIT) {
          if (ii[r] < N) {
            float* dst = part + (long long)c * 3 * N + ii[r];
            dst[0] = px[r], dst[N] = py[r], dst[2 * N] = pz[r];
          }
        } else {
          tx[r] = tx[r] + px[r], ty[r] = ty[r] + py[r], tz[r] = tz[r] + pz[r];
        }
      }
    }
    if (!SPLIT) {
#pragma unroll
      for (int r = 0; r < TS_R; ++r)
        if (ii[r] < N) {
          reinterpret_cast<float2*>(rep)[ii[r]] = float2{tx[r], ty[r]};
          z[ii[r]] = tz[r];
        }
    }
  }
}

// the chunks' partials in ascending chunk order, from zero: the additions of the unsplit kernel
__global__ __launch_bounds__(256) void tsne_repulsion_finish_kernel(const float* __restrict__ part, long long N, int nchunks, float* __restrict__ rep,
                                                                    float* __restrict__ z) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const float* src = part + (long long)c * 3 * N + i;
    tx = tx + src[0], ty = ty + src[N], tz = tz + src[2 * N];
  }
  reinterpret_cast<float2*>(rep)[i] = float2{tx, ty};
  z[i] = tz;
}

__global__ __launch_bounds__(256) void tsne_step_kernel(const float2* __restrict__ y, const float2* __restrict__ rep, const float* __restrict__ zsum,
                                                        const long long* __restrict__ offsets, const int* __restrict__ cols,
                                                        const float* __restrict__ vals, long long N, float exaggeration, float momentum, float lr,
                                                        float min_gain, float2* __restrict__ update, float2* __restrict__ gains,
                                                        float2* __restrict__ y_out, float* __restrict__ kl_rows, float2* __restrict__ att) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;   // (no barrier below)
  const float2 yi = y[i];
  const long long beg = offsets[i], end = offsets[i + 1];
  float ax = 0.f, ay = 0.f, kl = 0.f;
  for (long long e = beg + lane; e < end; e += 64) {
    const int c = cols[e];
    const float2 yj = y[c < 0 ? 0 : (c < N ? c : N - 1)];   // (a column outside 0 .. N-1 is read inside the allocation)
    const float v = vals[e];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float d = fmaf(dx, dx, fmaf(dy, dy, 1.f));
    const float w = v * __builtin_amdgcn_rcpf(d);
    ax = fmaf(w, dx, ax);
    ay = fmaf(w, dy, ay);
    if (kl_rows && v > 0.f) kl = fmaf(v, logf(v) + logf(d), kl);   // log v - log q, q = 1 / d
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (kl_rows) kl = wave_sum(kl);
  if (lane != 0) return;
  const float Z = zsum[0];
  const float2 r = rep[i];
  const float rx = Z > 0.f ? r.x / Z : 0.f, ry = Z > 0.f ? r.y / Z : 0.f;
  const float g[2] = {4.f * fmaf(exaggeration, ax, -rx), 4.f * fmaf(exaggeration, ay, -ry)};
  const float2 u = update[i], gn = gains[i];
  float un[2] = {u.x, u.y}, gg[2] = {gn.x, gn.y};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    gg[a] = fmaxf(un[a] * g[a] < 0.f ? gg[a] + 0.2f : gg[a] * 0.8f, min_gain);
    un[a] = fmaf(momentum, un[a], -(lr * (gg[a] * g[a])));
  }
  gains[i] = float2{gg[0], gg[1]};
  update[i] = float2{un[0], un[1]};
  y_out[i] = float2{yi.x + un[0], yi.y + un[1]};
  if (kl_rows) kl_rows[i] = kl;
  if (att) att[i] = float2{ax, ay};
}

int coati_tsne_affinities(const float* d2, const int32_t* nbr, int64_t N, int k, float perplexity, int steps, float* p, float* beta,
                          void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(d2, "tsne_affinities: d2 is null");
  COATI_CHECK_ARG(nbr, "tsne_affinities: nbr is null");
  COATI_CHECK_ARG(p, "tsne_affinities: p is null");
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "tsne_affinities: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(k >= 1 && k <= TS_K_MAX, "tsne_affinities: k=%d outside 1 .. %d", k, TS_K_MAX);
  COATI_CHECK_SHAPE(perplexity > 0.f && perplexity <= FLT_MAX, "tsne_affinities: perplexity=%g is not positive and finite", (double)perplexity);
  COATI_CHECK_SHAPE(steps >= 0 && steps <= 10000, "tsne_affinities: steps=%d outside 0 .. 10000", steps);
  hipLaunchKernelGGL(tsne_affinities_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, d2, nbr, N, k, logf(perplexity), steps, p, beta);
  COATI_LAUNCH_CHECK("tsne_affinities");
  return COATI_OK;
}

int coati_tsne_chunk(void) { return TS_J; }

int64_t coati_tsne_part_floats(int64_t N) {
  if (!(N >= 1 && N < (1ll << 31))) {
    coati_set_error("tsne_part_floats: N=%lld outside 1 .. 2^31 - 1", (long long)N);
    return COATI_ESHAPE;
  }
  return 3 * N * ((N + TS_J - 1) / TS_J);
}

int coati_tsne_repulsion(const float* y, int64_t N, float* rep, float* z, float* part, int64_t part_floats, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(y, "tsne_repulsion: y is null");
  COATI_CHECK_ARG(rep, "tsne_repulsion: rep is null");
  COATI_CHECK_ARG(z, "tsne_repulsion: z is null");
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "tsne_repulsion: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(blocks >= 0, "tsne_repulsion: blocks=%d < 0", blocks);
  COATI_CHECK_SHAPE(part_floats >= 0, "tsne_repulsion: part_floats=%lld < 0", (long long)part_floats);
  const long long tiles = (N + TS_TI - 1) / TS_TI;
  const int nchunks = (int)((N + TS_J - 1) / TS_J);
  const bool split = part && nchunks > 1 && tiles < TS_SPLIT_BELOW && part_floats >= 3 * N * nchunks;
  const long long items = split ? tiles * nchunks : tiles;
  const int grid = (int)(blocks > 0 && blocks < items ? blocks : (items < (1 << 20) ? items : (1 << 20)));
  const float2* y2 = reinterpret_cast<const float2*>(y);
  if (split) {
    hipLaunchKernelGGL(tsne_repulsion_kernel<true>, dim3(grid), dim3(256), 0, s, y2, N, rep, z, part, nchunks, items);
    COATI_LAUNCH_CHECK("tsne_repulsion");
    hipLaunchKernelGGL(tsne_repulsion_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, part, N, nchunks, rep, z);
    COATI_LAUNCH_CHECK("tsne_repulsion_finish");
  } else {
    hipLaunchKernelGGL(tsne_repulsion_kernel<false>, dim3(grid), dim3(256), 0, s, y2, N, rep, z, part, nchunks, items);
    COATI_LAUNCH_CHECK("tsne_repulsion");
  }
  return COATI_OK;
}

int coati_tsne_step(const float* y, const float* rep, const float* zsum, const int64_t* offsets, const int32_t* cols, const float* vals,
                    int64_t N, float exaggeration, float momentum, float lr, float min_gain, float* update, float* gains, float* y_out,
                    float* kl_rows, float* att, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(y, "tsne_step: y is null");
  COATI_CHECK_ARG(rep, "tsne_step: rep is null");
  COATI_CHECK_ARG(zsum, "tsne_step: zsum is null");
  COATI_CHECK_ARG(offsets, "tsne_step: offsets is null");
  COATI_CHECK_ARG(update, "tsne_step: update is null");
  COATI_CHECK_ARG(gains, "tsne_step: gains is null");
  COATI_CHECK_ARG(y_out, "tsne_step: y_out is null");
  COATI_CHECK_ARG(y_out != y, "tsne_step: y_out is y (other rows read y: use two buffers in turn)");
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "tsne_step: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  // (cols and vals may be null when P has no entry at all: no row then reads them)
  hipLaunchKernelGGL(tsne_step_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const float2*>(y),
                     reinterpret_cast<const float2*>(rep), zsum, LL(offsets), cols, vals, N, exaggeration, momentum, lr, min_gain,
                     reinterpret_cast<float2*>(update), reinterpret_cast<float2*>(gains), reinterpret_cast<float2*>(y_out), kl_rows,
                     reinterpret_cast<float2*>(att));
  COATI_LAUNCH_CHECK("tsne_step");
  return COATI_OK;
}
