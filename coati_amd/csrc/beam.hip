// Beam search over the KV-cached decode path (include/coati_beam.h): attention that follows beam ancestry instead of copying cache
// rows, and the selection of the W best of W x V continuations per embedding by cumulative log-probability.
//
// A session of B = G * W rows serves G embeddings with W beams each (row g * W + r).  After every step the surviving beams are a
// permutation-with-repeats of the previous ones.  A cache record (row, t) is written once and never changes, so the rows do not move:
// anc[b][t] names the cache row that holds position t of beam b's history, at 4 extra bytes per 64 / 128-B record read.
#include "../../include/coati_beam.h"
#include "decode_dev.h"

// The cached (row, head) sequence that holds position t of beam b: row anc[b * Tmax + t] (an entry outside 0 .. B - 1 reads row b).  A
// lane reads its table entries t = lane + 64 i coalesced, then the records.
__device__ __forceinline__ const bf16_t* anc_seq(const bf16_t* cache, const int* __restrict__ anc, int b, int h, int t, int B, int n_head,
                                                 int Tmax, int rec) {
  int r = anc[(long long)b * Tmax + t];
  r = (r >= 0 && r < B) ? r : b;
  return cache + (((long long)r * n_head + h) * Tmax) * rec;
}

// attn_decode_kernel<DHS, false> (decode.hip) with the records of t < pos read through the ancestry table: the same text
// (attn_decode_body.inc), so the same arithmetic statement for statement; the new record still goes to (b, pos).
template <int DHS>
__global__ __launch_bounds__(256) void attn_decode_anc_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                              bf16_t* __restrict__ y, int B, int n_head, int Tmax, int pos_arg,
                                                              const int* __restrict__ anc) {
  constexpr bool ROWS = false;
  const int* const pos_dev = nullptr;
#define ATTN_DECODE_SEQ(t) anc_seq(cache, anc, b, h, t, B, n_head, Tmax, REC)
#include "attn_decode_body.inc"
#undef ATTN_DECODE_SEQ
}

int launch_attn_decode_anc(const bf16_t* qkv, bf16_t* cache, bf16_t* y, int B, int n_head, int head_size, int Tmax, int pos,
                           const int* anc, hipStream_t s) {
  COATI_CHECK_ARG(qkv && cache && y, "attn_decode_anc: null operand");
  COATI_CHECK_ARG(anc, "attn_decode_anc: null ancestry table");
  COATI_CHECK_SHAPE(B > 0 && n_head > 0 && Tmax > 0 && Tmax <= 256 && pos >= 0 && pos < Tmax && (head_size == 16 || head_size == 32),
                    "attn_decode_anc: unsupported shape B=%d nh=%d hs=%d Tmax=%d pos=%d", B, n_head, head_size, Tmax, pos);
  if (head_size == 16)
    hipLaunchKernelGGL(attn_decode_anc_kernel<16>, dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, pos, anc);
  else
    hipLaunchKernelGGL(attn_decode_anc_kernel<32>, dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, pos, anc);
  COATI_LAUNCH_CHECK("attn_decode_anc");
  return COATI_OK;
}

#define BEAM_MAX 16

// One workgroup per row b of the [B = G * W, V] logits: the row's W best continuations as (cum[b] + log_softmax(logits[b])[tok], tok),
// best first (logit descending, token ascending).  lse = max + log(sum exp(x - max)) with accurate expf / logf in a fixed order: thread
// i sums its entries i, i + 256, ... in index order, then a binary tree over the 256 partials.
// fin[b] != 0: one candidate (cum[b], pad_token) -- a finished hypothesis continues as itself -- and W - 1 of score -inf.
// cum[b] == -inf gives -inf only: the first step starts every group from cum = [0, -inf, ...], and W identical rows then yield the W
// distinct continuations of row 0.
__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ logits, long long ldl, int W, int V,
                                                            const float* __restrict__ cum, const int* __restrict__ fin, int pad_token,
                                                            float* __restrict__ cand_score, int* __restrict__ cand_tok) {
  extern __shared__ unsigned keys[];   // [V]
  __shared__ TopkLds sm;
  __shared__ float red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float c = cum[b];
  float* out_s = cand_score + (long long)b * W;
  int* out_t = cand_tok + (long long)b * W;
  if (fin[b]) {
    if (tid < W) {
      out_s[tid] = tid == 0 ? c : -INFINITY;
      out_t[tid] = pad_token;
    }
    return;
  }
  const float* lrow = logits + (long long)b * ldl;
  topk_select_row(lrow, V, W, keys, sm);
  const float mx = key2f(sm.top_k[0]);
  float part = 0.f;
  for (int i = tid; i < V; i += 256) part += expf(key2f(keys[i]) - mx);   // (the row's logits, from LDS)
  red[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const float lse = mx + logf(red[0]);
  if (tid < W) {
    out_s[tid] = c + (key2f(sm.top_k[tid]) - lse);
    out_t[tid] = sm.top_i[tid];
  }
}

int coati_beam_row_topk(const float* logits, int64_t ldl, int G, int W, int V, const float* cum, const int32_t* fin, int pad_token,
                        float* cand_score, int32_t* cand_tok, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(logits && cum && fin && cand_score && cand_tok, "beam_row_topk: null operand");
  COATI_CHECK_SHAPE(G > 0 && W >= 1 && W <= BEAM_MAX && V > 0 && W <= V && (size_t)V * 4 <= 120 * 1024 && ldl >= V &&
                        (long long)G * W <= 0x7fffffffLL,
                    "beam_row_topk: unsupported shape G=%d W=%d V=%d ldl=%lld (1 <= W <= %d, W <= V)", G, W, V, (long long)ldl, BEAM_MAX);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(beam_row_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    if (e != hipSuccess) {
      coati_set_error("beam_row_topk: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(beam_row_topk_kernel, dim3(G * W), dim3(256), (size_t)V * 4, s, logits, ldl, W, V, cum, fin, pad_token, cand_score, cand_tok);
  COATI_LAUNCH_CHECK("beam_row_topk");
  return COATI_OK;
}

// One workgroup per group g: its W * W <= 256 candidates (row p of the group contributes cand[(g * W + p) * W + j]) ranked with one
// candidate per thread, by counting.  Order: score descending, parent row ascending, token ascending (then the candidate's slot j, which
// only separates the -inf fillers of a finished row, so that the ranks are a permutation whatever the input); a NaN score ranks as -inf.
// The best W become the group's new rows g * W + rank.  For new row r with parent p (global row index) and token tok:
//   cum_out = the score, fin_out = fin_in[p] || tok == stop_token, len_out = len_in[p] + (fin_in[p] ? 0 : 1), tok_next = tok,
//   anc_out[r][0 .. pos-1] = anc_in[p][0 .. pos-1], anc_out[r][pos] = p      (pos = the position the last step appended at)
//   hist_out[r][0 .. n-1] = hist_in[p][0 .. n-1],   hist_out[r][n] = tok      (n = beam steps taken so far)
// anc / hist are ping-pong buffers of the caller.  Plain stores: one workgroup owns one group, parents never leave their group.
// nfin[g] = the group's finished rows.
__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ cand_score, const int* __restrict__ cand_tok, int W,
                                                         const float* __restrict__ cum_in, const int* __restrict__ fin_in,
                                                         const int* __restrict__ len_in, const int* __restrict__ anc_in,
                                                         const long long* __restrict__ hist_in, long long ldh, int Tmax, int pos, int n,
                                                         int stop_token, float* __restrict__ cum_out, int* __restrict__ fin_out,
                                                         int* __restrict__ len_out, int* __restrict__ anc_out,
                                                         long long* __restrict__ hist_out, long long* __restrict__ tok_next,
                                                         int* __restrict__ nfin) {
  __shared__ float s_sc[BEAM_MAX * BEAM_MAX];
  __shared__ int s_tok[BEAM_MAX * BEAM_MAX];
  __shared__ int sel_p[BEAM_MAX], sel_tok[BEAM_MAX], sel_fin[BEAM_MAX];
  const int g = blockIdx.x, tid = threadIdx.x, n_cand = W * W;
  const long long row0 = (long long)g * W;
  if (tid < n_cand) {
    const float sc = cand_score[row0 * W + tid];
    s_sc[tid] = (sc != sc) ? -INFINITY : sc;
    s_tok[tid] = cand_tok[row0 * W + tid];
  }
  __syncthreads();
  if (tid < n_cand) {
    const float sc = s_sc[tid];
    const int tok = s_tok[tid], p = tid / W;
    int rank = 0;
    for (int j = 0; j < n_cand; ++j) {
      const float sj = s_sc[j];
      const int tj = s_tok[j], pj = j / W;
      const bool before = sj > sc || (sj == sc && (pj < p || (pj == p && (tj < tok || (tj == tok && j < tid)))));
      rank += before ? 1 : 0;
    }
    if (rank < W) {
      const long long r = row0 + rank, pr = row0 + p;
      const int f = fin_in[pr];
      const int fo = (f || tok == stop_token) ? 1 : 0;
      cum_out[r] = sc;
      fin_out[r] = fo;
      len_out[r] = len_in[pr] + (f ? 0 : 1);
      tok_next[r] = tok;
      sel_p[rank] = (int)pr;
      sel_tok[rank] = tok;
      sel_fin[rank] = fo;
    }
  }
  __syncthreads();
  for (int r = 0; r < W; ++r) {
    const long long pr = sel_p[r];
    const int* ai = anc_in + pr * Tmax;
    int* ao = anc_out + (row0 + r) * Tmax;
    for (int t = tid; t < pos; t += 256) ao[t] = ai[t];
    const long long* hi = hist_in + pr * ldh;
    long long* ho = hist_out + (row0 + r) * ldh;
    for (int i = tid; i < n; i += 256) ho[i] = hi[i];
    if (tid == 0) {
      ao[pos] = (int)pr;
      ho[n] = sel_tok[r];
    }
  }
  if (tid == 0) {
    int c = 0;
    for (int r = 0; r < W; ++r) c += sel_fin[r];
    nfin[g] = c;
  }
}

int coati_beam_merge(const float* cand_score, const int32_t* cand_tok, int G, int W, const float* cum_in, const int32_t* fin_in,
                     const int32_t* len_in, const int32_t* anc_in, const int64_t* hist_in, int64_t ldh, int Tmax, int pos, int n,
                     int stop_token, float* cum_out, int32_t* fin_out, int32_t* len_out, int32_t* anc_out, int64_t* hist_out,
                     int64_t* tok_next, int32_t* nfin, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(cand_score && cand_tok && cum_in && fin_in && len_in && anc_in && hist_in && cum_out && fin_out && len_out && anc_out &&
                      hist_out && tok_next && nfin,
                  "beam_merge: null operand");
  COATI_CHECK_ARG(anc_in != anc_out && hist_in != hist_out && cum_in != cum_out && fin_in != fin_out && len_in != len_out,
                  "beam_merge: the in and out buffers must differ (ping-pong)");
  COATI_CHECK_SHAPE(G > 0 && W >= 1 && W <= BEAM_MAX && (long long)G * W <= 0x7fffffffLL && Tmax > 0 && pos >= 0 && pos < Tmax && n >= 0 &&
                        n < ldh,
                    "beam_merge: unsupported shape G=%d W=%d Tmax=%d pos=%d n=%d ldh=%lld (1 <= W <= %d, pos < Tmax, n < ldh)", G, W, Tmax,
                    pos, n, (long long)ldh, BEAM_MAX);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(G), dim3(256), 0, s, cand_score, cand_tok, W, cum_in, fin_in, len_in, anc_in, LL(hist_in), ldh, Tmax,
                     pos, n, stop_token, cum_out, fin_out, len_out, anc_out, LL(hist_out), LL(tok_next), nfin);
  COATI_LAUNCH_CHECK("beam_merge");
  return COATI_OK;
}
