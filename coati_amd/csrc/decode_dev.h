// Device code shared by decode.hip and beam.hip: the radix selection of a logits row's k largest entries and the bf16 record load.
// (The attention body the two units share is attn_decode_body.inc.)
#pragma once
#include "kernels.h"

template <int N>
__device__ __forceinline__ void load_bf16(const bf16_t* p, float* x) {
#pragma unroll
  for (int i = 0; i < N / 8; ++i) unpack8(*reinterpret_cast<const uint4*>(p + 8 * i), x + 8 * i);
}

// ---- selection of a row's k largest logits ------------------------------------------------------------------------------
#define TOPK_MAX 128
__device__ __forceinline__ unsigned f2key(float f) {   // larger float <-> larger unsigned (NaN sorts high, like torch)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// LDS of one row's selection (the row's keys themselves live in the kernel's dynamic LDS, [V])
struct TopkLds {
  int hist[256];
  unsigned prefix;
  int need, ngt, neq;
  unsigned top_k[TOPK_MAX];
  int top_i[TOPK_MAX];
};

// The k largest entries of ONE row (the workgroup's 256 threads, all of them; k <= TOPK_MAX, k <= V): on return sm.top_k[0 .. k-1] are
// their order-preserving keys and sm.top_i their indices, key descending, index ascending (the order of a stable descending sort),
// visible to every thread.  keys: [V] of LDS.  The k-th largest key is found with a 4-pass radix select (8 bits per pass, one histogram
// bin per thread), the survivors are compacted (ties at the threshold in index order) and ranked by counting.
__device__ __forceinline__ void topk_select_row(const float* __restrict__ lrow, int V, int k, unsigned* keys, TopkLds& sm) {
  const int tid = threadIdx.x;
  for (int i = tid; i < V; i += 256) keys[i] = f2key(lrow[i]);
  if (tid == 0) { sm.prefix = 0u; sm.need = k; }
  __syncthreads();
  // radix select of the k-th largest key: after pass p the top 8*(p+1) bits of the threshold are known
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    sm.hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = sm.prefix;
    for (int i = tid; i < V; i += 256) {
      const unsigned key = keys[i];
      if ((key & mask) == prefix) atomicAdd(&sm.hist[(key >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int need = sm.need, bin = 255;
      for (; bin > 0; --bin) {
        if (sm.hist[bin] >= need) break;
        need -= sm.hist[bin];
      }
      sm.need = need;                              // rank of the threshold inside its bin
      sm.prefix = prefix | ((unsigned)bin << shift);
    }
    __syncthreads();
  }
  const unsigned tau = sm.prefix;                  // the k-th largest key; sm.need = how many keys == tau belong to the top k
  if (tid == 0) { sm.ngt = 0; sm.neq = 0; }
  __syncthreads();
  // survivors: every key > tau (any order), then the first sm.need keys == tau in index order
  for (int i = tid; i < V; i += 256) {
    if (keys[i] > tau) {
      const int slot = atomicAdd(&sm.ngt, 1);
      sm.top_k[slot] = keys[i];
      sm.top_i[slot] = i;
    }
  }
  __syncthreads();
  {
    // the first sm.need keys == tau in INDEX order: threads own contiguous index segments, exclusive scan of their counts
    const int seg = (V + 255) / 256, i0 = tid * seg, i1 = (i0 + seg < V) ? i0 + seg : V;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += (keys[i] == tau) ? 1 : 0;
    sm.hist[tid] = cnt;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < tid; ++t) before += sm.hist[t];
    const int base = sm.ngt, need = sm.need;
    if (cnt > 0 && before < need) {
      int pos = before;
      for (int i = i0; i < i1 && pos < need; ++i)
        if (keys[i] == tau) { sm.top_k[base + pos] = tau; sm.top_i[base + pos] = i; ++pos; }
    }
  }
  __syncthreads();
  // sort the k survivors: key descending, index ascending (rank by counting; k <= 128)
  unsigned myk = 0;
  int myi = 0, rank = 0;
  if (tid < k) {
    myk = sm.top_k[tid];
    myi = sm.top_i[tid];
    for (int j = 0; j < k; ++j) {
      const unsigned kj = sm.top_k[j];
      const int ij = sm.top_i[j];
      rank += (kj > myk || (kj == myk && ij < myi)) ? 1 : 0;
    }
  }
  __syncthreads();
  if (tid < k) { sm.top_k[rank] = myk; sm.top_i[rank] = myi; }
  __syncthreads();
}
