// Product-quantised library search (include/coati_pq.h): a row of a bf16 library [N, E] as M = E / 8 code bytes, codes[n][m] naming the
// entry of code book m ([256] entries of 8 bf16) that stands for dimensions 8 m .. 8 m + 7 -- 16 times fewer bytes than the bf16 row --
// an encoder, and the streaming top-k over the codes with the code books in LDS.
//
// pq_encode_kernel, persistent workgroups of 4 waves over blocks of 64 rows, the whole code book (512 E bytes) in LDS, loaded once per
// workgroup.  A LANE is a row of the block and a WAVE a sub-space (m = wave, wave + 4, ...): all 64 lanes of a wave read the same entry
// of the code book at the same time, which the LDS serves as one broadcast, where lanes on different sub-spaces would be 4096 bytes
// apart and on one bank.  The distance is the header's expression, every operation rounded to f32 on its own (no fused multiply-add:
// the contraction is switched off for the function), entries in ascending order and a strict <, so the lowest index wins among equals.
// x is read once, 16 bytes per (row, sub-space).
//
// pq_topk_kernel<KSMAX, NP>, grid = (tiles of 16 NP queries) x (S slices), 4 waves -- the exact search's geometry (search.hip), its
// write-out and its merge.  A workgroup copies the code book into LDS once, loads its query tile's B fragments and runs pq_stream
// (pq_stream_dev.h: topk_stream with the operand read from the code book) over its slice.  LDS, all of it dynamic: the code book
// (512 E bytes), the lists [16 NP][cap] of 8-byte keys, then counts, thresholds and the two flags (PQ_WORDS_BYTES).  NP = 2 up to
// E = 128 (a fragment read from LDS then feeds two MFMAs), NP = 1 above, where the code book leaves room for 16 lists only.
#include "../../include/coati_pq.h"
#include "pq_stream_dev.h"
#include "search_host.h"

#define PQ_E_MAX 256
#define PQ_LDS_BYTES (160 * 1024)   // a CU's LDS, which one workgroup may take whole
#define PQ_WORDS_BYTES(NP) (16 * (NP) * 8 + 8)   // counts and thresholds [16 NP], flags [2]
#define PQ_SLICE_ROWS_MIN 16384     // a slice's code bytes (E / 8 a row) are at least 4 times the 512 E bytes of code book its workgroup loads
#define PQ_ENCODE_ROWS 64           // rows per block of the encoder: one per lane

static inline int pq_np(int E) { return E <= 128 ? 2 : 1; }
static inline size_t pq_lds(int E, int k) { return (size_t)512 * E + (size_t)16 * pq_np(E) * (k + 2 * TOPK_ROWS_IT) * sizeof(topk_key_t) + PQ_WORDS_BYTES(pq_np(E)); }

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_encode_kernel(const bf16_t* __restrict__ x, long long n, int E, const bf16_t* __restrict__ codebook,
                                                        unsigned char* __restrict__ codes) {
#pragma clang fp contract(off)
  extern __shared__ uint4 pq_cb[];   // [M][256]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, M = E >> 3;
  for (int i = tid; i < M * 256; i += 256) pq_cb[i] = reinterpret_cast<const uint4*>(codebook)[i];
  __syncthreads();
  const long long blocks = (n + PQ_ENCODE_ROWS - 1) / PQ_ENCODE_ROWS;
  for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {   // (no barrier inside)
    const long long row = b * PQ_ENCODE_ROWS + lane;
    if (row >= n) continue;
    for (int m = wave; m < M; m += 4) {
      const uint4 w = *reinterpret_cast<const uint4*>(x + row * E + 8 * m);
      const unsigned ww[4] = {w.x, w.y, w.z, w.w};
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(ww[i] << 16);
        v[2 * i + 1] = __uint_as_float(ww[i] & 0xffff0000u);
      }
      float best = INFINITY;
      int arg = 0;
      for (int e = 0; e < 256; ++e) {
        const uint4 c = pq_cb[m * 256 + e];   // the wave's: one address, a broadcast
        const unsigned cc[4] = {c.x, c.y, c.z, c.w};
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t0 = v[2 * i] - __uint_as_float(cc[i] << 16);
          const float t1 = v[2 * i + 1] - __uint_as_float(cc[i] & 0xffff0000u);
          const float p0 = t0 * t0, p1 = t1 * t1;
          d = i == 0 ? p0 + p1 : (d + p0) + p1;
        }
        if (d < best) {
          best = d;
          arg = e;
        }
      }
      codes[row * M + m] = (unsigned char)arg;
    }
  }
}

static int pq_check_E(const char* what, int E) {
  COATI_CHECK_SHAPE(E >= 32 && E <= PQ_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, PQ_E_MAX);
  return COATI_OK;
}

int coati_pq_encode(const uint16_t* x, int64_t n, int E, const uint16_t* codebook, uint8_t* codes, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x && codebook && codes, "pq_encode: null operand");
  COATI_TRY(pq_check_E("pq_encode", E));
  COATI_CHECK_SHAPE(n >= 1 && n < (1ll << 31), "pq_encode: n=%lld outside 1 .. 2^31 - 1", (long long)n);
  COATI_TRY(max_dynamic_lds<pq_encode_kernel>("pq_encode", 512 * PQ_E_MAX));
  const long long blocks = (n + PQ_ENCODE_ROWS - 1) / PQ_ENCODE_ROWS;
  hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), (size_t)512 * E, s, x, n, E, codebook, codes);
  COATI_LAUNCH_CHECK("pq_encode");
  return COATI_OK;
}

// ---- the stream over the codes -----------------------------------------------------------------------------------------------------------
template <int KSMAX, int NP>
__global__ __launch_bounds__(256) void pq_topk_kernel(const unsigned char* __restrict__ codes, long long N, int E, const bf16_t* __restrict__ codebook,
                                                      const float* __restrict__ bias, const bf16_t* __restrict__ q, int Q, int k, float alpha, int S,
                                                      long long slice_rows, int cap, float* __restrict__ part_score, int* __restrict__ part_row) {
  extern __shared__ uint4 pq_lds_base[];   // code book [E / 8][256] x 16 B | lists [16 NP][cap] x 8 B | counts | thresholds | flags
  uint4* cb = pq_lds_base;
  topk_key_t* sbuf = reinterpret_cast<topk_key_t*>(cb + 32 * E);
  int* s_cnt = reinterpret_cast<int*>(sbuf + 16 * NP * cap);
  float* s_thr = reinterpret_cast<float*>(s_cnt + 16 * NP);
  int* s_flag = reinterpret_cast<int*>(s_thr + 16 * NP);
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4);
  const long long r_begin = (long long)slice * slice_rows, r_end = min(N, r_begin + slice_rows);

  if (r_end > r_begin)   // (workgroup-uniform; a slice past the end gathers nothing)
    for (int i = tid; i < 32 * E; i += 256) cb[i] = reinterpret_cast<const uint4*>(codebook)[i];   // pq_stream's first barrier is behind this

  // the query tile: B[k = 32 s + 8 g + j][column = col] of panel p
  bf16x8 bq[NP][KSMAX];
  bool stored[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
    stored[p] = qi < Q;
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks && stored[p]) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + 32 * s + 8 * g);
      bq[p][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  pq_stream<KSMAX, NP>(codes, N, E, cb, bias, bq, np, stored, r_begin, r_end, alpha, k, cap, sbuf, s_cnt, s_thr, s_flag);
  topk_write_out(sbuf, s_cnt, cap, k, min(16 * np, Q - q0), ((long long)q0 * S + slice) * k, (long long)S * k, [](int row) { return row; },
                 part_score, part_row);
}

// The largest k of the scan at this E: 128 where the code book, the lists of 16 NP queries at cap = k + 2 TOPK_ROWS_IT and the words fit
// the CU's 160 KiB, else 64 (E = 256: 128 KiB + 24 KiB + 136 B); a negative code for an E outside the limits
int coati_pq_k_max(int E) {
  COATI_TRY(pq_check_E("pq_k_max", E));
  for (int k = TOPK_MAX; k >= 64; k /= 2)
    if (pq_lds(E, k) <= PQ_LDS_BYTES) return k;
  coati_set_error("pq_k_max: no k fits E=%d", E);   // (not reached within the limits)
  return COATI_ESHAPE;
}

static int pq_check(const char* what, long long N, int E, int Q, int k) {
  COATI_TRY(pq_check_E(what, E));
  COATI_CHECK_SHAPE(k >= 1 && k <= coati_pq_k_max(E), "%s: k=%d outside 1 .. %d at E=%d", what, k, coati_pq_k_max(E), E);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "%s: N=%lld outside 1 .. 2^31 - 1", what, N);
  COATI_CHECK_SHAPE(Q >= 1, "%s: Q=%d < 1", what, Q);
  return COATI_OK;
}

template <int KSMAX, int NP>
static int pq_launch(const unsigned char* codes, long long N, int E, const bf16_t* codebook, const float* bias, const bf16_t* q, int Q, int k,
                     float alpha, int S, float* part_score, int* part_row, hipStream_t s) {
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  const size_t lds = pq_lds(E, k);        // <= PQ_LDS_BYTES: k <= coati_pq_k_max(E)
  COATI_TRY((max_dynamic_lds<pq_topk_kernel<KSMAX, NP>>("pq_topk", PQ_LDS_BYTES)));
  hipLaunchKernelGGL((pq_topk_kernel<KSMAX, NP>), dim3(cdiv(Q, 16 * NP), S), dim3(256), lds, s, codes, N, E, codebook, bias, q, Q, k, alpha, S,
                     topk_slice_rows(N, S), cap, part_score, part_row);
  COATI_LAUNCH_CHECK("pq_topk");
  return COATI_OK;
}

int coati_pq_topk(const uint8_t* codes, int64_t N, int E, const uint16_t* codebook, const float* bias, const uint16_t* q, int Q, int k,
                  float alpha, int S, float* part_score, int32_t* part_row, float* out_score, int64_t* out_row, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(codes && codebook && q && part_score && part_row && out_score && out_row, "pq_topk: null operand");
  COATI_TRY(pq_check("pq_topk", N, E, Q, k));
  COATI_CHECK_SHAPE(S >= 1 && (long long)S * k <= TOPK_MERGE_MAX, "pq_topk: S=%d slices of k=%d exceed S * k <= %d", S, k, TOPK_MERGE_MAX);
  if (pq_np(E) == 2)
    COATI_TRY((pq_launch<4, 2>(codes, N, E, codebook, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  else
    COATI_TRY((pq_launch<8, 1>(codes, N, E, codebook, bias, q, Q, k, alpha, S, part_score, part_row, s)));
  return launch_search_merge(part_score, part_row, Q, S * k, k, out_score, LL(out_row), s);
}

// The number of slices coati_pq_topk is given by default: enough workgroups to fill the device at this Q (as many per CU as their LDS
// allows), no slice shorter than PQ_SLICE_ROWS_MIN rows unless the library is, S * k within the merge's row.  Host arithmetic only.
int coati_pq_slices(int64_t N, int E, int Q, int k) {
  COATI_TRY(pq_check("pq_slices", N, E, Q, k));
  const long long tiles = ((long long)Q + 16 * pq_np(E) - 1) / (16 * pq_np(E));
  const long long slots = 256 * (long long)(PQ_LDS_BYTES / pq_lds(E, k));
  const long long by_rows = (N + PQ_SLICE_ROWS_MIN - 1) / PQ_SLICE_ROWS_MIN, by_merge = TOPK_MERGE_MAX / k;
  long long S = (slots + tiles - 1) / tiles;
  S = S < by_rows ? S : by_rows;
  S = S < by_merge ? S : by_merge;
  return (int)(S > 1 ? S : 1);
}
