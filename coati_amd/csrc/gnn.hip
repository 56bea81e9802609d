// E(3)-GNN point encoder kernels (reference e3gnn_clip.py:108-137, e_gcl_sparse.py:10-77, 169-215, 253-321).
//
// MI355X formulation: the neighbour list is a dense, masked [B, A, A] edge grid built once per step on the
// device (coordinates never change across the 5 layers; the reference rebuilds it 5x with host syncs).
// Edge (b, j, k): receiver j, sender k, row index (b*A + j)*A + k, weight w = cubic_cutoff(d) * valid.
// The 513->256 edge Linear is factored  W1 [h_j, h_k, d^2] = W1a h_j + W1b h_k + w1c d^2, so its big part is a
// node-level MFMA GEMM (P = h [W1a;W1b]^T) and the per-edge part is the gather-add below.
// All kernels here are HBM/L2-bound gathers and segmented reductions: coalesced rows, no atomics on the
// per-edge path (messages are grouped by receiver), fp32 maths, bf16 storage for GEMM operands.
#include "kernels.h"

#define IN_EPS 1e-5f

// ---- atom embedding + instance norm ------------------------------------------------------------------------
// e = W[:, ix] + W[:, iy] + b  (the 28-wide one-hot times Linear(28,H)), h = (e - mean) / sqrt(var + eps)
__global__ __launch_bounds__(256) void gnn_embed_kernel(const long long* __restrict__ atoms, const int* __restrict__ lut_ix,
                                                        const int* __restrict__ lut_iy, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ h32,
                                                        bf16_t* __restrict__ h16, long long ld16, float* __restrict__ rstd_out,
                                                        float* __restrict__ mask, int BA, int H, int* __restrict__ err) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= BA) return;
  long long z = atoms[row];
  if (lane == 0) mask[row] = z > 0 ? 1.f : 0.f;
  // torch_emb: nn.Embedding(84, H) has no row for Z > 83 (the reference asserts / raises there, e3gnn_clip.py:113-115): bit 2 of the
  // step's error word -- the update is dropped and the host raises -- instead of silently training on row 83
  if (lut_ix == nullptr && z > 83 && lane == 0 && err != nullptr) atomicOr(err, 4);
  if (z < 0) z = 0;
  if (z > 119) z = 119;
  // lut_ix == nullptr: torch_emb (e3gnn_clip.py:49-56, 113-115) -- W is nn.Embedding(84, H)'s table, the row of the atomic number IS the
  // node feature (embedding = Identity, no bias)
  const bool table = lut_ix == nullptr;
  if (table && z > 83) z = 83;
  const int ix = table ? 0 : lut_ix[z], iy = table ? 0 : lut_iy[z];
  float e[16];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    float v = 0.f;
    if (c < H) {
      if (table) {
        v = W[z * H + c];
      } else {
        v = bias[c];
        if (ix >= 0) v += W[c * 28 + ix];
        if (iy >= 0) v += W[c * 28 + iy];
      }
    }
    e[i] = v;
    s += v;
  }
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (lane + 64 * i < H) q += (e[i] - mean) * (e[i] - mean);
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + IN_EPS);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    if (c < H) {
      const float v = (e[i] - mean) * rstd;
      h32[(long long)row * H + c] = v;
      h16[(long long)row * ld16 + c] = f2bf(v);
    }
  }
}

int launch_gnn_embed(const long long* atoms, const int* lut_ix, const int* lut_iy, const float* W, const float* b,
                     float* h32, bf16_t* h16, long long ld16, float* rstd, float* mask, int BA, int H,
                     hipStream_t s, int* err) {
  COATI_CHECK_ARG(atoms && W && h32 && h16 && rstd && mask && ((lut_ix && lut_iy && b) || (!lut_ix && !lut_iy && !b)), "gnn_embed: null operand");
  COATI_CHECK_SHAPE(BA > 0 && H > 0 && H <= 1024, "gnn_embed: unsupported shape");
  hipLaunchKernelGGL(gnn_embed_kernel, dim3(cdiv(BA, 4)), dim3(256), 0, s, atoms, lut_ix, lut_iy, W, b, h32, h16, ld16, rstd, mask, BA, H, err);
  COATI_LAUNCH_CHECK("gnn_embed");
  return COATI_OK;
}

// dW[:, i] = sum over atoms whose one-hot has bit i of de[atom, :]; db = sum over all atoms.
// One pass over de: a workgroup owns a chunk of atoms, thread = channel, the 28 + 1 partial sums per channel live in LDS
// ([29][H] floats, own column per thread -> no LDS atomics needed); the flush walks dW in memory order so consecutive
// lanes add to consecutive addresses.
__global__ __launch_bounds__(256) void gnn_embed_bwd_kernel(const long long* __restrict__ atoms, const int* __restrict__ lut_ix,
                                                            const int* __restrict__ lut_iy, const float* __restrict__ de,
                                                            float* __restrict__ dW, float* __restrict__ db, int BA, int H,
                                                            int rows_per_chunk) {
  extern __shared__ float acc[];   // [29][H]
  for (int i = threadIdx.x; i < 29 * H; i += blockDim.x) acc[i] = 0.f;
  __syncthreads();
  const int r0 = blockIdx.x * rows_per_chunk;
  int r1 = r0 + rows_per_chunk;
  if (r1 > BA) r1 = BA;
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float bsum = 0.f;
    for (int row = r0; row < r1; ++row) {
      long long z = atoms[row];
      if (z < 0) z = 0;
      if (z > 119) z = 119;
      const int ix = lut_ix[z], iy = lut_iy[z];
      const float v = de[(long long)row * H + c];
      bsum += v;
      if (ix >= 0) acc[ix * H + c] += v;                // (iy = -1: the actinides, whose period bit overflows the 28-wide one-hot --
      if (iy >= 0 && iy != ix) acc[iy * H + c] += v;    // gnn_embed_kernel adds no column for it; the guards of gnn_onehot_wgrad_kernel)
    }
    acc[28 * H + c] = bsum;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < 28 * H; f += blockDim.x) {   // f = c * 28 + i: the memory order of dW [H][28]
    const int c = f / 28, i = f - c * 28;
    const float v = acc[i * H + c];
    if (v != 0.f) atomicAdd(dW + f, v);
  }
  for (int c = threadIdx.x; c < H; c += blockDim.x) atomicAdd(db + c, acc[28 * H + c]);
}

// torch_emb: dTable[z, :] += de[atom, :] over the atoms of atomic number z (nn.Embedding's backward).  A workgroup owns a chunk of atoms,
// thread = channel; runs of equal atomic numbers are summed in a register before the atomic (hydrogens and carbons come in runs)
__global__ __launch_bounds__(256) void gnn_embed_table_bwd_kernel(const long long* __restrict__ atoms, const float* __restrict__ de,
                                                                  float* __restrict__ dT, int BA, int H, int rows_per_chunk) {
  const int r0 = blockIdx.x * rows_per_chunk;
  int r1 = r0 + rows_per_chunk;
  if (r1 > BA) r1 = BA;
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float run = 0.f;
    long long zr = -1;
    for (int row = r0; row < r1; ++row) {
      long long z = atoms[row];
      if (z < 0) z = 0;
      if (z > 83) z = 83;
      if (z != zr) {
        if (zr >= 0 && run != 0.f) atomicAdd(dT + zr * H + c, run);
        zr = z;
        run = 0.f;
      }
      run += de[(long long)row * H + c];
    }
    if (zr >= 0 && run != 0.f) atomicAdd(dT + zr * H + c, run);
  }
}

int launch_gnn_embed_bwd(const long long* atoms, const int* lut_ix, const int* lut_iy, const float* de,
                         float* dW, float* db, int BA, int H, hipStream_t s) {
  if (lut_ix == nullptr && lut_iy == nullptr && db == nullptr) {   // torch_emb
    COATI_CHECK_ARG(atoms && de && dW, "gnn_embed_bwd: null operand");
    const int rpc = 32;
    hipLaunchKernelGGL(gnn_embed_table_bwd_kernel, dim3(cdiv(BA, rpc)), dim3(256), 0, s, atoms, de, dW, BA, H, rpc);
    COATI_LAUNCH_CHECK("gnn_embed_table_bwd");
    return COATI_OK;
  }
  COATI_CHECK_ARG(atoms && lut_ix && lut_iy && de && dW && db, "gnn_embed_bwd: null operand");
  COATI_CHECK_SHAPE((size_t)29 * H * 4 <= 64 * 1024, "gnn_embed_bwd: H=%d too wide for the LDS accumulator", H);
  const int chunks = BA >= 4096 ? 128 : (BA >= 256 ? 8 : 1);
  const int rpc = cdiv(BA, chunks);
  hipLaunchKernelGGL(gnn_embed_bwd_kernel, dim3(cdiv(BA, rpc)), dim3(256), (size_t)29 * H * 4, s, atoms, lut_ix, lut_iy, de, dW, db, BA, H, rpc);
  COATI_LAUNCH_CHECK("gnn_embed_bwd");
  return COATI_OK;
}

// ---- residual = True (e3gnn_clip.py:97-100, e_gcl_sparse.py:141, 282-290): every node MLP also sees the one-hot node features h0 ---------
// u = [h | mi] W3[:, :2H]^T + b3 comes from the GEMM (f32); the h0 columns of W3 are one-hot gathers: u += W3[:, 2H + ix] + W3[:, 2H + iy].
// Then what EPI_SILU would have written: the pre-activation (bf16, for the backward) and silu(u) (bf16, the next product's operand).
__global__ __launch_bounds__(256) void gnn_node_res_silu_kernel(const float* __restrict__ u32, const long long* __restrict__ atoms,
                                                                const int* __restrict__ lut_ix, const int* __restrict__ lut_iy,
                                                                const float* __restrict__ W3c, long long ldw, bf16_t* __restrict__ upre,
                                                                bf16_t* __restrict__ t16, int BA, int H) {
  const int row = blockIdx.x;
  if (row >= BA) return;
  long long z = atoms[row];
  if (z < 0) z = 0;
  if (z > 119) z = 119;
  const int ix = lut_ix[z], iy = lut_iy[z];
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float v = u32[(long long)row * H + c];
    if (ix >= 0) v += W3c[c * ldw + ix];
    if (iy >= 0 && iy != ix) v += W3c[c * ldw + iy];   // (group and period indices live in disjoint ranges; the guard mirrors gnn_onehot_wgrad_kernel)
    upre[(long long)row * H + c] = f2bf(v);
    t16[(long long)row * H + c] = f2bf(silu_f(v));
  }
}

int launch_gnn_node_res_silu(const float* u32, const long long* atoms, const int* lut_ix, const int* lut_iy, const float* W3c, long long ldw,
                             bf16_t* upre, bf16_t* t16, int BA, int H, hipStream_t s) {
  COATI_CHECK_ARG(u32 && atoms && lut_ix && lut_iy && W3c && upre && t16, "gnn_node_res_silu: null operand");
  hipLaunchKernelGGL(gnn_node_res_silu_kernel, dim3(BA), dim3(256), 0, s, u32, atoms, lut_ix, lut_iy, W3c, ldw, upre, t16, BA, H);
  COATI_LAUNCH_CHECK("gnn_node_res_silu");
  return COATI_OK;
}

// dW3[:, 2H + i] += sum over the atoms whose one-hot has bit i of du[atom, :] (du bf16, dW3 rows ldw apart): gnn_embed_bwd_kernel's scheme
__global__ __launch_bounds__(256) void gnn_onehot_wgrad_kernel(const long long* __restrict__ atoms, const int* __restrict__ lut_ix,
                                                               const int* __restrict__ lut_iy, const bf16_t* __restrict__ du,
                                                               float* __restrict__ dW, long long ldw, int BA, int H, int rows_per_chunk) {
  extern __shared__ float acc[];   // [28][H]
  for (int i = threadIdx.x; i < 28 * H; i += blockDim.x) acc[i] = 0.f;
  __syncthreads();
  const int r0 = blockIdx.x * rows_per_chunk;
  int r1 = r0 + rows_per_chunk;
  if (r1 > BA) r1 = BA;
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    for (int row = r0; row < r1; ++row) {
      long long z = atoms[row];
      if (z < 0) z = 0;
      if (z > 119) z = 119;
      const int ix = lut_ix[z], iy = lut_iy[z];
      const float v = bf2f(du[(long long)row * H + c]);
      if (ix >= 0) acc[ix * H + c] += v;
      if (iy >= 0 && iy != ix) acc[iy * H + c] += v;
    }
  }
  __syncthreads();
  for (int f = threadIdx.x; f < 28 * H; f += blockDim.x) {
    const int c = f / 28, i = f - c * 28;
    const float v = acc[i * H + c];
    if (v != 0.f) atomicAdd(dW + c * ldw + i, v);
  }
}

int launch_gnn_onehot_wgrad(const long long* atoms, const int* lut_ix, const int* lut_iy, const bf16_t* du, float* dW, long long ldw, int BA,
                            int H, hipStream_t s) {
  COATI_CHECK_ARG(atoms && lut_ix && lut_iy && du && dW, "gnn_onehot_wgrad: null operand");
  COATI_CHECK_SHAPE((size_t)28 * H * 4 <= 64 * 1024, "gnn_onehot_wgrad: H=%d too wide for the LDS accumulator", H);
  const int chunks = BA >= 4096 ? 128 : (BA >= 256 ? 8 : 1);
  const int rpc = cdiv(BA, chunks);
  hipLaunchKernelGGL(gnn_onehot_wgrad_kernel, dim3(cdiv(BA, rpc)), dim3(256), (size_t)28 * H * 4, s, atoms, lut_ix, lut_iy, du, dW, ldw, BA, H, rpc);
  COATI_LAUNCH_CHECK("gnn_onehot_wgrad");
  return COATI_OK;
}

// ---- geometry: squared distances and smooth-cutoff edge weights ---------------------------------------------------
__global__ void gnn_geom_kernel(const float* __restrict__ coords, const float* __restrict__ mask, float rc,
                                float* __restrict__ d2o, float* __restrict__ wo, int B, int A) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)B * A * A;
  if (e >= n) return;
  const int k = (int)(e % A);
  const long long bj = e / A;
  const int j = (int)(bj % A);
  const long long b = bj / A;
  const float* xj = coords + (b * A + j) * 3;
  const float* xk = coords + (b * A + k) * 3;
  const float dx = xj[0] - xk[0], dy = xj[1] - xk[1], dz = xj[2] - xk[2];
  const float d2 = dx * dx + dy * dy + dz * dz;
  const float d = sqrtf(d2);
  const bool valid = (mask[b * A + j] > 0.f) && (mask[b * A + k] > 0.f) && (j != k) && (d < rc);
  float w = 0.f;
  if (valid) {
    // e_gcl_sparse.py:10-24: 1 - 1.5 (r/rc)^2 + 0.5 (r/rc)^3 on (0, rc); 1 at r <= 0
    const float c2 = -1.5f / (rc * rc), c3 = 0.5f / (rc * rc * rc);
    w = (d <= 0.f) ? 1.f : (1.f + c2 * d * d + c3 * d * d * d);
  }
  d2o[e] = d2;
  wo[e] = w;
}

int launch_gnn_geom(const float* coords, const float* mask, float cutoff, float* d2, float* w, int B, int A,
                    hipStream_t s) {
  COATI_CHECK_ARG(coords && mask && d2 && w, "gnn_geom: null operand");
  const long long n = (long long)B * A * A;
  hipLaunchKernelGGL(gnn_geom_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, coords, mask, cutoff, d2, w, B, A);
  COATI_LAUNCH_CHECK("gnn_geom");
  return COATI_OK;
}

// =====================================================================================================================
// Compacted edge list.  make_neighborlist (e_gcl_sparse.py:27-77) keeps only the pairs inside the cutoff; a dense [B, A, A]
// grid (round 1; its edge kernels were deleted in round 4) computes every slot: with n ~ U{8..16} atoms per 16-slot molecule
// and 85 % of the pairs inside 5 A, 56 % of its rows are padding or out of range.  The list is built on the device from the
// dense weights of gnn_geom (w > 0 <=> edge), receiver-major, so that every per-receiver sum is a contiguous segment and
// nothing is atomic; its length never visits the host (the edge-level GEMMs read it through GemmArgs::m_dev).
// =====================================================================================================================
__global__ void gnn_compact_count_kernel(const float* __restrict__ w, int* __restrict__ cnt, int BA, int A) {
  const int bj = blockIdx.x * blockDim.x + threadIdx.x;
  if (bj >= BA) return;
  int n = 0;
  for (int k = 0; k < A; ++k) n += w[(long long)bj * A + k] > 0.f;
  cnt[bj] = n;
}
// exclusive scan of cnt[0..n) -> seg[0..n], seg[n] = total (one workgroup; n is a few ten thousand)
__global__ __launch_bounds__(1024) void gnn_scan_kernel(const int* __restrict__ cnt, int* __restrict__ seg, int* __restrict__ total, int n) {
  // per-thread run of `per` consecutive counts -> inclusive scan of the thread sums inside each wave (6 shuffles) -> scan of the 16
  // wave totals by the first wave: two workgroup barriers (the 10-step shared-memory scan of round 2 had twenty: 21 us)
  __shared__ int wtot[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, per = (n + 1023) / 1024;
  const int lo = t * per, hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += cnt[i];
  int incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    int w = lane < 16 ? wtot[lane] : 0;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const int v = __shfl_up(w, off, 64);
      if (lane >= off) w += v;
    }
    if (lane < 16) wtot[lane] = w;     // inclusive totals of waves 0 .. lane
  }
  __syncthreads();
  int run = incl - s + (wave > 0 ? wtot[wave - 1] : 0);
  for (int i = lo; i < hi; ++i) { seg[i] = run; run += cnt[i]; }
  if (t == 1023) { seg[n] = wtot[15]; total[0] = wtot[15]; }
}
__global__ void gnn_compact_fill_kernel(const float* __restrict__ w, const float* __restrict__ d2, const int* __restrict__ seg,
                                        int* __restrict__ e_bj, int* __restrict__ e_bk, float* __restrict__ e_d2,
                                        float* __restrict__ e_w, int* __restrict__ pos, int BA, int A) {
  const int bj = blockIdx.x * blockDim.x + threadIdx.x;
  if (bj >= BA) return;
  const int b = bj / A;
  int e = seg[bj];
  for (int k = 0; k < A; ++k) {
    const long long slot = (long long)bj * A + k;
    const float ww = w[slot];
    if (ww > 0.f) {
      e_bj[e] = bj; e_bk[e] = b * A + k; e_d2[e] = d2[slot]; e_w[e] = ww;
      pos[slot] = e++;
    }
  }
}
__global__ void gnn_compact_rev_kernel(const int* __restrict__ n_edges, const int* __restrict__ e_bj, const int* __restrict__ e_bk,
                                       const int* __restrict__ pos, int* __restrict__ e_rev, int A) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges[0]) return;
  const int bj = e_bj[e], bk = e_bk[e];
  e_rev[e] = pos[(long long)bk * A + (bj % A)];   // slot of (receiver k, sender j): the same molecule, the same distance
}
int launch_gnn_compact(const float* w_dense, const float* d2_dense, int* seg, int* n_edges, int* e_bj, int* e_bk, int* e_rev,
                       float* e_d2, float* e_w, int* pos, int B, int A, hipStream_t s) {
  COATI_CHECK_ARG(w_dense && d2_dense && seg && n_edges && e_bj && e_bk && e_rev && e_d2 && e_w && pos, "gnn_compact: null operand");
  COATI_CHECK_SHAPE(B > 0 && A > 0 && (long long)B * A * A < (1LL << 31), "gnn_compact: B*A*A must fit 31 bits");   // any A: the *_c kernels walk a receiver's segment in 64-edge chunks
  const int BA = B * A;
  // the per-receiver counts are parked in e_rev (B*A*A ints, rewritten by the last pass)
  hipLaunchKernelGGL(gnn_compact_count_kernel, dim3(cdiv(BA, 256)), dim3(256), 0, s, w_dense, e_rev, BA, A);
  hipLaunchKernelGGL(gnn_scan_kernel, dim3(1), dim3(1024), 0, s, e_rev, seg, n_edges, BA);
  hipLaunchKernelGGL(gnn_compact_fill_kernel, dim3(cdiv(BA, 256)), dim3(256), 0, s, w_dense, d2_dense, seg, e_bj, e_bk, e_d2, e_w, pos, BA, A);
  hipLaunchKernelGGL(gnn_compact_rev_kernel, dim3(cdiv((long long)BA * A, 256)), dim3(256), 0, s, n_edges, e_bj, e_bk, pos, e_rev, A);
  COATI_LAUNCH_CHECK("gnn_compact");
  return COATI_OK;
}

// edge layer 1 on the list: one wave per receiver, looping over its segment
__global__ __launch_bounds__(256) void gnn_edge_pre_c_kernel(const bf16_t* __restrict__ P, long long ldp, const int* __restrict__ seg,
                                                             const int* __restrict__ e_bk, const float* __restrict__ e_d2,
                                                             const float* __restrict__ w1c, long long w1c_stride,
                                                             const float* __restrict__ b1, bf16_t* __restrict__ e1, int BA, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bj = blockIdx.x * 4 + wave;
  if (bj >= BA) return;
  const int e0 = seg[bj], n = seg[bj + 1] - e0;
  // every lane walks the loop (H < 256 leaves lanes without channels): the segment metadata is read with readlane from
  // ALL 64 lanes, so the loads that fill it must not sit in divergent control flow; lanes without channels compute on
  // channel 0 and store nothing
  for (int c0 = 0; c0 < H; c0 += 256) {
    const bool act = c0 + lane * 4 < H;
    const int c = act ? c0 + lane * 4 : 0;
    const uint2 ua = *reinterpret_cast<const uint2*>(P + (long long)bj * ldp + c);
    const float pa[4] = {bflo(ua.x), bfhi(ua.x), bflo(ua.y), bfhi(ua.y)};
    float wc[4], bb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { wc[i] = w1c[(long long)(c + i) * w1c_stride]; bb[i] = b1[c + i]; }
    // the segment's sender rows and distances: one coalesced load per wave and 64-edge chunk, broadcast with readlane
    // (one chunk whenever the molecule has at most 64 atoms)
    for (int base = 0; base < n; base += 64) {
      const int nn = n - base < 64 ? n - base : 64;
      const int my_bk = lane < nn ? e_bk[e0 + base + lane] : 0;
      const float my_d2 = lane < nn ? e_d2[e0 + base + lane] : 0.f;
      for (int i0 = 0; i0 < nn; i0 += 4) {
        uint2 ub[4];
        float dd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u < nn ? i0 + u : nn - 1;
          const int bk = __builtin_amdgcn_readlane(my_bk, i);
          dd[u] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_d2), i));
          ub[u] = *reinterpret_cast<const uint2*>(P + (long long)bk * ldp + H + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (i0 + u >= nn) break;
          const float pb[4] = {bflo(ub[u].x), bfhi(ub[u].x), bflo(ub[u].y), bfhi(ub[u].y)};
          float o[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = silu_f(pa[i] + pb[i] + dd[u] * wc[i] + bb[i]);
          if (act) *reinterpret_cast<uint2*>(e1 + (long long)(e0 + base + i0 + u) * H + c) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
        }
      }
    }
  }
}
int launch_gnn_edge_pre_c(const bf16_t* P, long long ldp, const int* seg, const int* e_bk, const float* e_d2, const float* w1c,
                          long long w1c_stride, const float* b1, bf16_t* e1, int BA, int H, hipStream_t s) {
  COATI_CHECK_ARG(P && seg && e_bk && e_d2 && w1c && b1 && e1, "gnn_edge_pre_c: null operand");
  COATI_CHECK_SHAPE(H % 4 == 0 && ldp % 4 == 0, "gnn_edge_pre_c: alignment");
  hipLaunchKernelGGL(gnn_edge_pre_c_kernel, dim3(cdiv(BA, 4)), dim3(256), 0, s, P, ldp, seg, e_bk, e_d2, w1c, w1c_stride, b1, e1, BA, H);
  COATI_LAUNCH_CHECK("gnn_edge_pre_c");
  return COATI_OK;
}

// mi[bj,:] = sum over the receiver's segment of SiLU(s2[e,:]) * w[e]
__global__ __launch_bounds__(256) void gnn_edge_reduce_c_kernel(const bf16_t* __restrict__ s2, const int* __restrict__ seg,
                                                                const float* __restrict__ e_w, bf16_t* __restrict__ mi,
                                                                long long ldmi, int BA, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bj = blockIdx.x * 4 + wave;
  if (bj >= BA) return;
  const int e0 = seg[bj], n = seg[bj + 1] - e0;
  // every lane walks the loop (H < 256 leaves lanes without channels): the segment metadata is read with readlane from
  // ALL 64 lanes, so the loads that fill it must not sit in divergent control flow; lanes without channels compute on
  // channel 0 and store nothing
  for (int c0 = 0; c0 < H; c0 += 256) {
    const bool act = c0 + lane * 4 < H;
    const int c = act ? c0 + lane * 4 : 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < n; base += 64) {
      const int nn = n - base < 64 ? n - base : 64;
      const float my_w = lane < nn ? e_w[e0 + base + lane] : 0.f;
      for (int i0 = 0; i0 < nn; i0 += 4) {
        uint2 u[4];
        float ww[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + q < nn ? i0 + q : nn - 1;
          ww[q] = i0 + q < nn ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), i)) : 0.f;
          u[q] = *reinterpret_cast<const uint2*>(s2 + (long long)(e0 + base + i) * H + c);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[0] += silu_f(bflo(u[q].x)) * ww[q]; acc[1] += silu_f(bfhi(u[q].x)) * ww[q];
          acc[2] += silu_f(bflo(u[q].y)) * ww[q]; acc[3] += silu_f(bfhi(u[q].y)) * ww[q];
        }
      }
    }
    if (act) *reinterpret_cast<uint2*>(mi + (long long)bj * ldmi + c) = make_uint2(pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]));
  }
}
int launch_gnn_edge_reduce_c(const bf16_t* s2, const int* seg, const float* e_w, bf16_t* mi, long long ldmi, int BA, int H, hipStream_t s) {
  COATI_CHECK_ARG(s2 && seg && e_w && mi, "gnn_edge_reduce_c: null operand");
  COATI_CHECK_SHAPE(H % 4 == 0 && ldmi % 4 == 0, "gnn_edge_reduce_c: alignment");
  hipLaunchKernelGGL(gnn_edge_reduce_c_kernel, dim3(cdiv(BA, 4)), dim3(256), 0, s, s2, seg, e_w, mi, ldmi, BA, H);
  COATI_LAUNCH_CHECK("gnn_edge_reduce_c");
  return COATI_OK;
}

// ds2[e,:] = dmi[receiver(e),:] * w[e] * SiLU'(s2[e,:])
__global__ __launch_bounds__(256) void gnn_edge_reduce_bwd_c_kernel(const bf16_t* __restrict__ dmi, long long lddmi,
                                                                    const bf16_t* __restrict__ s2, const int* __restrict__ seg,
                                                                    const float* __restrict__ e_w, bf16_t* __restrict__ ds2, int BA, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bj = blockIdx.x * 4 + wave;
  if (bj >= BA) return;
  const int e0 = seg[bj], n = seg[bj + 1] - e0;
  // every lane walks the loop (H < 256 leaves lanes without channels): the segment metadata is read with readlane from
  // ALL 64 lanes, so the loads that fill it must not sit in divergent control flow; lanes without channels compute on
  // channel 0 and store nothing
  for (int c0 = 0; c0 < H; c0 += 256) {
    const bool act = c0 + lane * 4 < H;
    const int c = act ? c0 + lane * 4 : 0;
    const uint2 ug = *reinterpret_cast<const uint2*>(dmi + (long long)bj * lddmi + c);
    const float g[4] = {bflo(ug.x), bfhi(ug.x), bflo(ug.y), bfhi(ug.y)};
    for (int base = 0; base < n; base += 64) {
      const int nn = n - base < 64 ? n - base : 64;
      const float my_w = lane < nn ? e_w[e0 + base + lane] : 0.f;
      for (int i0 = 0; i0 < nn; i0 += 4) {
        uint2 u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = *reinterpret_cast<const uint2*>(s2 + (long long)(e0 + base + (i0 + q < nn ? i0 + q : nn - 1)) * H + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (i0 + q >= nn) break;
          const float ww = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), i0 + q));
          if (act) *reinterpret_cast<uint2*>(ds2 + (long long)(e0 + base + i0 + q) * H + c) =
              make_uint2(pack2bf(g[0] * ww * dsilu_f(bflo(u[q].x)), g[1] * ww * dsilu_f(bfhi(u[q].x))),
                         pack2bf(g[2] * ww * dsilu_f(bflo(u[q].y)), g[3] * ww * dsilu_f(bfhi(u[q].y))));
        }
      }
    }
  }
}
int launch_gnn_edge_reduce_bwd_c(const bf16_t* dmi, long long lddmi, const bf16_t* s2, const int* seg, const float* e_w,
                                 bf16_t* ds2, int BA, int H, hipStream_t s) {
  COATI_CHECK_ARG(dmi && s2 && seg && e_w && ds2, "gnn_edge_reduce_bwd_c: null operand");
  COATI_CHECK_SHAPE(H % 4 == 0 && lddmi % 4 == 0, "gnn_edge_reduce_bwd_c: alignment");
  hipLaunchKernelGGL(gnn_edge_reduce_bwd_c_kernel, dim3(cdiv(BA, 4)), dim3(256), 0, s, dmi, lddmi, s2, seg, e_w, ds2, BA, H);
  COATI_LAUNCH_CHECK("gnn_edge_reduce_bwd_c");
  return COATI_OK;
}

// backward of the gather-add on the list: dPa[bj] = sum over the receiver's segment of dpre[e]; dPb[bj] = the same sum over
// the REVERSE edges (sender bj: rows e_rev[e]), dw1c += sum dpre[e] d2[e], db1 += sum dpre[e].  Persistent workgroups: the
// two column sums stay in registers across receivers, one atomic per channel and workgroup.
#define EPB_WAVES 16   // waves per workgroup: the loads of a receiver are a latency chain, so the CU needs many receivers in flight; the
                       // number of WORKGROUPS (= atomics per channel) stays at 512
__global__ __launch_bounds__(64 * EPB_WAVES) void gnn_edge_pre_bwd_c_kernel(const bf16_t* __restrict__ dpre, const int* __restrict__ seg,
                                                                 const int* __restrict__ e_rev, const float* __restrict__ e_d2,
                                                                 bf16_t* __restrict__ dP, long long lddp, float* __restrict__ dw1c,
                                                                 long long dw1c_stride, float* __restrict__ db1, int BA, int H) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // every lane walks the loop (H < 256 leaves lanes without channels): the segment metadata is read with readlane from
  // ALL 64 lanes, so the loads that fill it must not sit in divergent control flow; lanes without channels compute on
  // channel 0 and store nothing
  for (int c0 = 0; c0 < H; c0 += 256) {
    const bool act = c0 + lane * 4 < H;
    const int c = act ? c0 + lane * 4 : 0;
    float sw[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int bj = blockIdx.x * EPB_WAVES + wave; bj < BA; bj += gridDim.x * EPB_WAVES) {
      const int e0 = seg[bj], n = seg[bj + 1] - e0;
      float a[4] = {0.f, 0.f, 0.f, 0.f}, bsum[4] = {0.f, 0.f, 0.f, 0.f};
      for (int base = 0; base < n; base += 64) {
        const int nn = n - base < 64 ? n - base : 64;
        const int my_rev = lane < nn ? e_rev[e0 + base + lane] : 0;
        const float my_d2 = lane < nn ? e_d2[e0 + base + lane] : 0.f;
        for (int i0 = 0; i0 < nn; i0 += 4) {
          uint2 u[4], r[4];
          float dd[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool ok = i0 + q < nn;
            const int i = ok ? i0 + q : nn - 1;
            const int rv = __builtin_amdgcn_readlane(my_rev, i);
            dd[q] = ok ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_d2), i)) : 0.f;
            u[q] = *reinterpret_cast<const uint2*>(dpre + (long long)(e0 + base + i) * H + c);
            r[q] = *reinterpret_cast<const uint2*>(dpre + (long long)rv * H + c);
            if (!ok) { u[q] = make_uint2(0, 0); r[q] = make_uint2(0, 0); }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float x[4] = {bflo(u[q].x), bfhi(u[q].x), bflo(u[q].y), bfhi(u[q].y)};
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] += x[i]; sw[i] = fmaf(x[i], dd[q], sw[i]); }
            bsum[0] += bflo(r[q].x); bsum[1] += bfhi(r[q].x); bsum[2] += bflo(r[q].y); bsum[3] += bfhi(r[q].y);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) sb[i] += a[i];
      if (act) {
        *reinterpret_cast<uint2*>(dP + (long long)bj * lddp + c) = make_uint2(pack2bf(a[0], a[1]), pack2bf(a[2], a[3]));
        *reinterpret_cast<uint2*>(dP + (long long)bj * lddp + H + c) = make_uint2(pack2bf(bsum[0], bsum[1]), pack2bf(bsum[2], bsum[3]));
      }
    }
    // column sums: the 4 waves of the workgroup add up through LDS, then ONE atomic per channel and workgroup (thousands of
    // same-address atomics serialise in the L2: 2048 workgroups x 4 waves made this kernel 1 ms)
    __shared__ float red[2][EPB_WAVES][256];
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[0][wave][lane * 4 + i] = act ? sw[i] : 0.f; red[1][wave][lane * 4 + i] = act ? sb[i] : 0.f; }
    __syncthreads();
    if (wave == 0 && act) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = lane * 4 + i;
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int w = 0; w < EPB_WAVES; ++w) { t0 += red[0][w][k]; t1 += red[1][w][k]; }
        atomicAdd(dw1c + (long long)(c + i) * dw1c_stride, t0);
        atomicAdd(db1 + c + i, t1);
      }
    }
    __syncthreads();
  }
}
int launch_gnn_edge_pre_bwd_c(const bf16_t* dpre, const int* seg, const int* e_rev, const float* e_d2, bf16_t* dP, long long lddp,
                              float* dw1c, long long dw1c_stride, float* db1, int BA, int H, hipStream_t s) {
  COATI_CHECK_ARG(dpre && seg && e_rev && e_d2 && dP && dw1c && db1, "gnn_edge_pre_bwd_c: null operand");
  COATI_CHECK_SHAPE(H % 4 == 0 && lddp % 4 == 0, "gnn_edge_pre_bwd_c: alignment");
  int blocks = cdiv(BA, EPB_WAVES);
  // ONE 16-wave workgroup per CU, each looping over its receivers.  Measured (gnn_elemwise per step): 64 workgroups 1.19 ms,
  // 128 / 256: 1.04, 512: 1.17, 1024: 1.44 -- and the same with the column sums taken out of the atomics (a two-stage form:
  // 1.05 / 1.17 / 1.36): it is the gathers of the reverse rows that degrade with more waves in flight, not the atomics
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(gnn_edge_pre_bwd_c_kernel, dim3(blocks), dim3(64 * EPB_WAVES), 0, s, dpre, seg, e_rev, e_d2, dP, lddp, dw1c, dw1c_stride, db1, BA, H);
  COATI_LAUNCH_CHECK("gnn_edge_pre_bwd_c");
  return COATI_OK;
}

// ---- masked mean readout (e3gnn_clip.py:134-137) and its backward ----------------------------------------------------
__global__ __launch_bounds__(256) void gnn_readout_kernel(const float* __restrict__ o, const float* __restrict__ mask,
                                                          float* __restrict__ hp, int A, int H) {
  const int b = blockIdx.x;
  float n = 0.f;
  for (int a = 0; a < A; ++a) n += mask[b * A + a];
  n = fmaxf(n, 1.f);
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    float acc = 0.f;
    for (int a = 0; a < A; ++a) acc += o[((long long)b * A + a) * H + c] * mask[b * A + a];
    hp[(long long)b * H + c] = acc / n;
  }
}

int launch_gnn_readout(const float* o, const float* mask, float* hp, int B, int A, int H, hipStream_t s) {
  COATI_CHECK_ARG(o && mask && hp, "gnn_readout: null operand");
  hipLaunchKernelGGL(gnn_readout_kernel, dim3(B), dim3(256), 0, s, o, mask, hp, A, H);
  COATI_LAUNCH_CHECK("gnn_readout");
  return COATI_OK;
}

__global__ __launch_bounds__(256) void gnn_readout_bwd_kernel(const float* __restrict__ dhp, const float* __restrict__ mask,
                                                              bf16_t* __restrict__ dout, int A, int H) {
  const int b = blockIdx.x;
  float n = 0.f;
  for (int a = 0; a < A; ++a) n += mask[b * A + a];
  n = fmaxf(n, 1.f);
  for (int c = threadIdx.x; c < H; c += blockDim.x) {
    const float g = dhp[(long long)b * H + c] / n;
    for (int a = 0; a < A; ++a) dout[((long long)b * A + a) * H + c] = f2bf(g * mask[b * A + a]);
  }
}

int launch_gnn_readout_bwd(const float* dhp, const float* mask, bf16_t* dout, int B, int A, int H, hipStream_t s) {
  COATI_CHECK_ARG(dhp && mask && dout, "gnn_readout_bwd: null operand");
  hipLaunchKernelGGL(gnn_readout_bwd_kernel, dim3(B), dim3(256), 0, s, dhp, mask, dout, A, H);
  COATI_LAUNCH_CHECK("gnn_readout_bwd");
  return COATI_OK;
}
