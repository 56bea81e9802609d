// The host side that the search units share (search.hip, search8.hip, search4.hip, pq.hip, radius.hip, ivf.hip, ivfpq.hip): the limits of
// the sliced top-k entries, the slices' arithmetic and the one-time raise of a kernel's dynamic-LDS limit.  Host code only: nothing here
// is called from, or changes, a kernel.
#pragma once
#include "topk_stream_dev.h"

#define TOPK_MERGE_MAX 30720     // S * k: one query's partial lists are search_merge_kernel's row of keys in 120 KiB of LDS
#define TOPK_DEVICE_SLOTS 512    // workgroups (IVF: work items) that fill the device: 256 CUs, two workgroups each where the LDS allows

// The rows of one of S slices of an N-row library: whole iterations, so a slice past the end of the library (S > N / TOPK_ROWS_IT) is
// empty -- it writes padding only, or has no hits.
static inline long long topk_slice_rows(long long N, int S) {
  return (N + (long long)S * TOPK_ROWS_IT - 1) / ((long long)S * TOPK_ROWS_IT) * TOPK_ROWS_IT;
}

// The limits the flat top-k entries share (`what`: the entry, for coati_last_error); the width E is the entry's own rule.
static inline int topk_check(const char* what, long long N, int Q, int k, int S) {
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX, "%s: k=%d outside 1 .. %d", what, k, TOPK_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "%s: N=%lld outside 1 .. 2^31 - 1", what, N);
  COATI_CHECK_SHAPE(Q >= 1, "%s: Q=%d < 1", what, Q);
  COATI_CHECK_SHAPE(S >= 1 && (long long)S * k <= TOPK_MERGE_MAX, "%s: S=%d slices of k=%d exceed S * k <= %d", what, S, k, TOPK_MERGE_MAX);
  return COATI_OK;
}

// The number of slices a flat top-k entry is given by default: enough workgroups to fill the device at this Q (tiles of 64 queries), no
// slice shorter than one workgroup iteration, S * k within the merge's row.  Host arithmetic only.
static inline int topk_default_slices(const char* what, long long N, int Q, int k) {
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX && N >= 1 && N < (1ll << 31) && Q >= 1, "%s: N=%lld Q=%d k=%d out of range", what, N, Q, k);
  const long long tiles = ((long long)Q + 63) / 64;
  const long long by_rows = (N + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT, by_merge = TOPK_MERGE_MAX / k;
  long long S = (TOPK_DEVICE_SLOTS + tiles - 1) / tiles;
  S = S < by_rows ? S : by_rows;
  S = S < by_merge ? S : by_merge;
  return (int)(S > 1 ? S : 1);
}

// Raises Kernel's dynamic-LDS limit to `bytes` (the most any launch of it asks for) the first time it is called: one flag per kernel.
template <auto Kernel>
static int max_dynamic_lds(const char* what, int bytes) {
  static bool raised = false;
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
      coati_set_error("%s: hipFuncSetAttribute(%d bytes of LDS) failed: %s", what, bytes, hipGetErrorString(e));
      return COATI_EHIP;
    }
    raised = true;
  }
  return COATI_OK;
}
