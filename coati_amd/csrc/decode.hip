// Inference decode step: KV-cached causal attention for ONE new token per sequence at
// head size 16, and top-k sampling of the next token (reference smiles_xformer.py:272-351 recomputes the whole prefix
// for every generated token; here the rotated keys and the values of earlier positions live in an HBM cache).
//
// Cache layout: [B][n_head][Tmax][k | v] bf16 (head size 16 or 32) -> one (b, head) sequence is a contiguous run of
// 64 / 128-B records, a wave streams it with one record per lane per pass.  HBM-bound: 4 * hs bytes per cached token
// per head per step.
#include "decode_dev.h"

// qkv: [B, 3C] bf16 of the new token (q, k already rotated by the QKV GEMM epilogue); y: [B, C] bf16.
// One wave per (b, head).  Appends (k, v) at position pos, attends to positions 0..pos.  ROWS (ragged sessions): row b sits at its own
// position pos_dev[b].  The body, with its commentary, is attn_decode_body.inc, shared with the ancestry-following kernel of
// beam.hip.
template <int DHS, bool ROWS>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                          bf16_t* __restrict__ y, int B, int n_head, int Tmax, int pos_arg,
                                                          const int* __restrict__ pos_dev) {
#define ATTN_DECODE_SEQ(t) seq
#include "attn_decode_body.inc"
#undef ATTN_DECODE_SEQ
}

__global__ void add_int_kernel(int* x, int v, int set) { *x = set ? v : *x + v; }
// set != 0: *x = v; else *x += v   (the decode position lives in device memory for graph replay)
int launch_add_int(int* x, int v, int set, hipStream_t s) {
  hipLaunchKernelGGL(add_int_kernel, dim3(1), dim3(1), 0, s, x, v, set);
  COATI_LAUNCH_CHECK("add_int");
  return COATI_OK;
}

int launch_attn_decode(const bf16_t* qkv, bf16_t* cache, bf16_t* y, int B, int n_head, int head_size, int Tmax, int pos,
                       const int* pos_dev, hipStream_t s) {
  COATI_CHECK_ARG(qkv && cache && y, "attn_decode: null operand");
  COATI_CHECK_SHAPE(B > 0 && n_head > 0 && Tmax > 0 && Tmax <= 256 && pos >= 0 && pos < Tmax && (head_size == 16 || head_size == 32),
                    "attn_decode: unsupported shape B=%d nh=%d hs=%d Tmax=%d pos=%d", B, n_head, head_size, Tmax, pos);
  if (head_size == 16)
    hipLaunchKernelGGL((attn_decode_kernel<16, false>), dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, pos, pos_dev);
  else
    hipLaunchKernelGGL((attn_decode_kernel<32, false>), dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, pos, pos_dev);
  COATI_LAUNCH_CHECK("attn_decode");
  return COATI_OK;
}

// Row b at its own position pos[b] (device, [B]); a position outside 0 .. Tmax - 1 = idle slot, untouched.
int launch_attn_decode_rows(const bf16_t* qkv, bf16_t* cache, bf16_t* y, int B, int n_head, int head_size, int Tmax, const int* pos,
                            hipStream_t s) {
  COATI_CHECK_ARG(qkv && cache && y && pos, "attn_decode_rows: null operand");
  COATI_CHECK_SHAPE(B > 0 && n_head > 0 && Tmax > 0 && Tmax <= 256 && (head_size == 16 || head_size == 32),
                    "attn_decode_rows: unsupported shape B=%d nh=%d hs=%d Tmax=%d", B, n_head, head_size, Tmax);
  if (head_size == 16)
    hipLaunchKernelGGL((attn_decode_kernel<16, true>), dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, 0, pos);
  else
    hipLaunchKernelGGL((attn_decode_kernel<32, true>), dim3(cdiv(B * n_head, 4)), dim3(256), 0, s, qkv, cache, y, B, n_head, Tmax, 0, pos);
  COATI_LAUNCH_CHECK("attn_decode_rows");
  return COATI_OK;
}

// The ragged step's per-row operands (one launch in front of the step):
//   rope_t[b]  = pos[b], or 0 for an idle slot: the QKV epilogue indexes its cos / sin tables with it for EVERY row of the product,
//                idle ones included, so it must always be a valid table row (never -1).  What an idle row then computes (from
//                whatever its token and buffers hold, possibly non-finite) is read by nobody: every product and LayerNorm of the step
//                is row-wise, and the attention returns before it touches an idle row.
//   tok_inj[b] = tokens[b] where the row may read the injection (inj_len == null: everywhere, else while pos[b] < inj_len[b]), else
//                -1, an id that never equals [UNK]: a row that SAMPLED the [UNK] id behind its prompt takes the table's embedding.
__global__ void decode_rows_prep_kernel(const int* __restrict__ pos, const int* __restrict__ inj_len, const long long* __restrict__ tokens,
                                        int* __restrict__ rope_t, long long* __restrict__ tok_inj, int B, int Tmax) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int p = pos[b];
  const bool live = p >= 0 && p < Tmax;
  rope_t[b] = live ? p : 0;
  tok_inj[b] = (live && (inj_len == nullptr || p < inj_len[b])) ? tokens[b] : -1;
}
int launch_decode_rows_prep(const int* pos, const int* inj_len, const long long* tokens, int* rope_t, long long* tok_inj, int B, int Tmax,
                            hipStream_t s) {
  COATI_CHECK_ARG(pos && tokens && rope_t && tok_inj, "decode_rows_prep: null operand");
  hipLaunchKernelGGL(decode_rows_prep_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, pos, inj_len, tokens, rope_t, tok_inj, B, Tmax);
  COATI_LAUNCH_CHECK("decode_rows_prep");
  return COATI_OK;
}

// ---- top-k sampling (smiles_xformer.py:305-313) -----------------------------------------------------------------------
//   logits_topk, inds = topk(logits[b], k);  probs = softmax(logits_topk * inv_temp);  token = inds[multinomial(probs)]
// One workgroup per row, the row's order-preserving integer keys in LDS.  The k-th largest key is found with a 4-pass
// radix select (8 bits per pass, one histogram bin per thread), the <= TOPK_MAX survivors are compacted (ties at the
// threshold in index order), sorted (value descending, index ascending -- the order of a stable descending sort) and
// sampled by inverse CDF with the caller's uniform u[b] in [0, 1).  stopped rows emit pad_token; a row that draws
// stop_token is marked stopped (reference :314-324).  Integer/compare work on a 40-KB row: ~10 us per row-block.
// The selection (topk_select_row, decode_dev.h: shared with beam.hip) and the draw for ONE row (the workgroup's 256 threads, all of
// them): returns the token in thread 0 (other threads: unspecified).  Shared by topk_sample_kernel and topk_sample_prompt_kernel, so
// that an unforced row of the second gives the very bits of the first.
__device__ __forceinline__ int topk_sample_row(const float* __restrict__ lrow, int V, int k, float inv_temp, float uval,
                                               unsigned* keys, TopkLds& sm) {
  const int tid = threadIdx.x;
  topk_select_row(lrow, V, k, keys, sm);
  int tok = 0;
  if (tid == 0) {
    const float mx = key2f(sm.top_k[0]) * inv_temp;
    float z = 0.f;
    int last = 0;   // the last candidate of non-zero weight: k - 1 on finite logits, fewer when a mask left fewer than k entries above -inf
    for (int r = 0; r < k; ++r) {
      const float w = __expf(key2f(sm.top_k[r]) * inv_temp - mx);
      z += w;
      last = w > 0.f ? r : last;
    }
    const float target = uval * z;
    float c = 0.f;
    int pick = last;   // (where rounding lets uval * z reach the running sum)
    for (int r = 0; r < k; ++r) {
      c += __expf(key2f(sm.top_k[r]) * inv_temp - mx);
      if (target < c) { pick = r; break; }
    }
    tok = sm.top_i[pick];
  }
  return tok;
}

__global__ __launch_bounds__(256) void topk_sample_kernel(const float* __restrict__ logits, long long ldl, int V, int k,
                                                          float inv_temp, const float* __restrict__ u,
                                                          long long* __restrict__ tok_out, int* __restrict__ stopped,
                                                          int stop_token, int pad_token) {
  extern __shared__ unsigned keys[];   // [V]
  __shared__ TopkLds sm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (stopped && stopped[b]) {
    if (tid == 0) tok_out[b] = pad_token;
    return;
  }
  const int tok = topk_sample_row(logits + (long long)b * ldl, V, k, inv_temp, u ? u[b] : 0.f, keys, sm);
  if (tid == 0) {
    tok_out[b] = tok;
    if (stopped && tok == stop_token) stopped[b] = 1;
  }
}

// Per-row prompts (completion of prompts of different lengths): at output position pos, row b with pos < plen[b] emits its own
// prompt token prompt[b, pos] (no draw; a [STOP] in the prompt flags the row); otherwise a stopped row emits pad_token and a live
// row samples exactly as topk_sample_kernel.
__global__ __launch_bounds__(256) void topk_sample_prompt_kernel(const float* __restrict__ logits, long long ldl, int V, int k,
                                                                 float inv_temp, const float* __restrict__ u,
                                                                 const long long* __restrict__ prompt, long long ldp,
                                                                 const int* __restrict__ plen, int pos,
                                                                 long long* __restrict__ tok_out, int* __restrict__ stopped,
                                                                 int stop_token, int pad_token) {
  extern __shared__ unsigned keys[];   // [V]
  __shared__ TopkLds sm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (pos < plen[b] && pos < ldp) {
    if (tid == 0) {
      const long long tok = prompt[(long long)b * ldp + pos];
      tok_out[b] = tok;
      if (stopped && tok == stop_token) stopped[b] = 1;
    }
    return;
  }
  if (stopped && stopped[b]) {
    if (tid == 0) tok_out[b] = pad_token;
    return;
  }
  const int tok = topk_sample_row(logits + (long long)b * ldl, V, k, inv_temp, u ? u[b] : 0.f, keys, sm);
  if (tid == 0) {
    tok_out[b] = tok;
    if (stopped && tok == stop_token) stopped[b] = 1;
  }
}

int launch_topk_sample(const float* logits, long long ldl, int B, int V, int k, float inv_temp, const float* u,
                       long long* tok_out, int* stopped, int stop_token, int pad_token, hipStream_t s) {
  COATI_CHECK_ARG(logits && tok_out, "topk_sample: null operand");
  COATI_CHECK_SHAPE(B > 0 && V > 0 && k > 0 && k <= TOPK_MAX && k <= V && (size_t)V * 4 <= 120 * 1024,
                    "topk_sample: unsupported shape B=%d V=%d k=%d", B, V, k);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    if (e != hipSuccess) {
      coati_set_error("topk_sample: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(topk_sample_kernel, dim3(B), dim3(256), (size_t)V * 4, s, logits, ldl, V, k, inv_temp, u, tok_out, stopped, stop_token, pad_token);
  COATI_LAUNCH_CHECK("topk_sample");
  return COATI_OK;
}

int launch_topk_sample_prompt(const float* logits, long long ldl, int B, int V, int k, float inv_temp, const float* u,
                              const long long* prompt, long long ldp, const int* plen, int pos, long long* tok_out, int* stopped,
                              int stop_token, int pad_token, hipStream_t s) {
  COATI_CHECK_ARG(logits && tok_out && prompt && plen, "topk_sample_prompt: null operand");
  COATI_CHECK_SHAPE(B > 0 && V > 0 && k > 0 && k <= TOPK_MAX && k <= V && (size_t)V * 4 <= 120 * 1024 && ldl >= V && ldp > 0 && pos >= 0,
                    "topk_sample_prompt: unsupported shape B=%d V=%d k=%d ldp=%lld pos=%d", B, V, k, ldp, pos);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_sample_prompt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    if (e != hipSuccess) {
      coati_set_error("topk_sample_prompt: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(topk_sample_prompt_kernel, dim3(B), dim3(256), (size_t)V * 4, s, logits, ldl, V, k, inv_temp, u, prompt, ldp, plen,
                     pos, tok_out, stopped, stop_token, pad_token);
  COATI_LAUNCH_CHECK("topk_sample_prompt");
  return COATI_OK;
}

// Ragged sessions (per-row positions): one workgroup per slot.  pos[b] is the position the step that produced logits[b] appended at
// (the cache holds n = pos[b] + 1 tokens); pos[b] < 0 = idle slot: nothing is read or written.  The slot serves request
// r = req ? req[b] : b, which selects its prompt row, prompt length, uniform and output row:
//   n < plen[r]  -> emits prompt[r, n] without a draw (a [STOP] there ends the row, as in topk_sample_prompt_kernel);
//   otherwise    -> draws with topk_sample_row (the very bits of topk_sample_kernel on the same logits and uniform); the uniform is
//                   u[b] (ldu == 0) or u[r * ldu + n]: a request's draws then depend on the request and the position alone.
// The token goes to out[r, n] and to tok_next[b] (the next step's token vector), pos[b] becomes n (the next step appends there), and
// the slot turns idle (pos[b] = -1, done[b] = n + 1 = the row's length) when the token is [STOP] or n is the last column (Tmax - 1).
// One workgroup owns one slot and distinct slots serve distinct requests: plain stores, no atomics.
__global__ __launch_bounds__(256) void topk_sample_rows_kernel(const float* __restrict__ logits, long long ldl, int V, int k,
                                                               float inv_temp, const float* __restrict__ u, long long ldu,
                                                               const long long* __restrict__ prompt, long long ldp,
                                                               const int* __restrict__ plen, const int* __restrict__ req,
                                                               int* __restrict__ pos, long long* __restrict__ out, long long ldo,
                                                               long long* __restrict__ tok_next, int* __restrict__ done, int Tmax,
                                                               int stop_token) {
  extern __shared__ unsigned keys[];   // [V]
  __shared__ TopkLds sm;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int p = pos[b];
  if (p < 0) return;
  const int n = p + 1;
  if (n >= Tmax || n >= ldo) {   // (a full row that was not retired: retire it, write nothing)
    if (tid == 0) { pos[b] = -1; done[b] = n; }
    return;
  }
  const long long r = req ? req[b] : b;
  long long tok;
  if (plen != nullptr && n < plen[r] && n < ldp) {
    tok = prompt[r * ldp + n];
  } else {
    tok = topk_sample_row(logits + (long long)b * ldl, V, k, inv_temp, u ? u[ldu > 0 ? r * ldu + n : b] : 0.f, keys, sm);
  }
  if (tid == 0) {
    out[r * ldo + n] = tok;
    tok_next[b] = tok;
    const bool end = tok == stop_token || n + 1 >= Tmax || n + 1 >= ldo;
    pos[b] = end ? -1 : n;
    if (end) done[b] = n + 1;
  }
}

int launch_topk_sample_rows(const float* logits, long long ldl, int B, int V, int k, float inv_temp, const float* u, long long ldu,
                            const long long* prompt, long long ldp, const int* plen, const int* req, int* pos, long long* out,
                            long long ldo, long long* tok_next, int* done, int Tmax, int stop_token, hipStream_t s) {
  COATI_CHECK_ARG(logits && pos && out && tok_next && done && (plen == nullptr || prompt != nullptr), "topk_sample_rows: null operand");
  COATI_CHECK_SHAPE(B > 0 && V > 0 && k > 0 && k <= TOPK_MAX && k <= V && (size_t)V * 4 <= 120 * 1024 && ldl >= V && ldu >= 0 &&
                        (plen == nullptr || ldp > 0) && ldo > 0 && Tmax > 0,
                    "topk_sample_rows: unsupported shape B=%d V=%d k=%d ldp=%lld ldo=%lld Tmax=%d", B, V, k, ldp, ldo, Tmax);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_sample_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    if (e != hipSuccess) {
      coati_set_error("topk_sample_rows: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(topk_sample_rows_kernel, dim3(B), dim3(256), (size_t)V * 4, s, logits, ldl, V, k, inv_temp, u, ldu, prompt, ldp, plen,
                     req, pos, out, ldo, tok_next, done, Tmax, stop_token);
  COATI_LAUNCH_CHECK("topk_sample_rows");
  return COATI_OK;
}

// ---- prompt prefill: the rotated keys and the values of a padded [B, m] pass into the decode cache ----------------------
// qkv: [B * m, 3C] bf16 (row b * m + t; q | k | v, q and k rotated by the QKV GEMM epilogue); cache: one layer's
// [B][nh][Tmax][k | v].  One thread per 16-B chunk of a record (2 * hs / 8 chunks), positions 0..m-1.
template <int DHS>
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache, int B, int m,
                                                            int n_head, int Tmax) {
  constexpr int CH = DHS / 8, REC = 2 * DHS;
  const long long n = (long long)B * n_head * m * 2 * CH;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % (2 * CH));
  const long long rec = i / (2 * CH);              // (b, h, t) with t fastest
  const int t = (int)(rec % m);
  const long long bh = rec / m;                    // b * n_head + h
  const int h = (int)(bh % n_head);
  const long long b = bh / n_head;
  const int C = n_head * DHS;
  const bf16_t* src = qkv + (b * m + t) * 3 * C + (c < CH ? C + h * DHS + c * 8 : 2 * C + h * DHS + (c - CH) * 8);
  *reinterpret_cast<uint4*>(cache + (bh * Tmax + t) * REC + c * 8) = *reinterpret_cast<const uint4*>(src);
}

int launch_kv_cache_fill(const bf16_t* qkv, bf16_t* cache, int B, int m, int n_head, int head_size, int Tmax, hipStream_t s) {
  COATI_CHECK_ARG(qkv && cache, "kv_cache_fill: null operand");
  COATI_CHECK_SHAPE(B > 0 && n_head > 0 && m > 0 && m <= Tmax && Tmax <= 256 && (head_size == 16 || head_size == 32),
                    "kv_cache_fill: unsupported shape B=%d nh=%d hs=%d m=%d Tmax=%d", B, n_head, head_size, m, Tmax);
  const long long n = (long long)B * n_head * m * (head_size / 4);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (head_size == 16)
    hipLaunchKernelGGL(kv_cache_fill_kernel<16>, grid, dim3(256), 0, s, qkv, cache, B, m, n_head, Tmax);
  else
    hipLaunchKernelGGL(kv_cache_fill_kernel<32>, grid, dim3(256), 0, s, qkv, cache, B, m, n_head, Tmax);
  COATI_LAUNCH_CHECK("kv_cache_fill");
  return COATI_OK;
}

// The same from a PACKED pass (ragged prefill: every row's own prompt length): row r of qkv [R, 3C] is slot row_src[r] = b * T + t of
// the padded [B, T] token matrix (embed.hip, the pass's row map) and goes to (b, t) of the cache.  One thread per 16-B chunk.
template <int DHS>
__global__ __launch_bounds__(256) void kv_cache_fill_rows_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                                 const int* __restrict__ row_src, int R, int B, int T, int n_head, int Tmax) {
  constexpr int CH = DHS / 8, REC = 2 * DHS;
  const long long n = (long long)R * n_head * 2 * CH;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % (2 * CH));
  const long long rec = i / (2 * CH);              // (r, h) with h fastest
  const int h = (int)(rec % n_head);
  const long long r = rec / n_head;
  const int slot = row_src[r];
  const int b = slot / T, t = slot - b * T;
  if (slot < 0 || b >= B || t >= Tmax) return;
  const int C = n_head * DHS;
  const bf16_t* src = qkv + r * 3 * C + (c < CH ? C + h * DHS + c * 8 : 2 * C + h * DHS + (c - CH) * 8);
  *reinterpret_cast<uint4*>(cache + (((long long)b * n_head + h) * Tmax + t) * REC + c * 8) = *reinterpret_cast<const uint4*>(src);
}

int launch_kv_cache_fill_rows(const bf16_t* qkv, bf16_t* cache, const int* row_src, int R, int B, int T, int n_head, int head_size,
                              int Tmax, hipStream_t s) {
  COATI_CHECK_ARG(qkv && cache && row_src, "kv_cache_fill_rows: null operand");
  COATI_CHECK_SHAPE(R > 0 && B > 0 && T > 0 && n_head > 0 && Tmax > 0 && Tmax <= 256 && (head_size == 16 || head_size == 32),
                    "kv_cache_fill_rows: unsupported shape R=%d B=%d T=%d nh=%d hs=%d Tmax=%d", R, B, T, n_head, head_size, Tmax);
  const long long n = (long long)R * n_head * (head_size / 4);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (head_size == 16)
    hipLaunchKernelGGL(kv_cache_fill_rows_kernel<16>, grid, dim3(256), 0, s, qkv, cache, row_src, R, B, T, n_head, Tmax);
  else
    hipLaunchKernelGGL(kv_cache_fill_rows_kernel<32>, grid, dim3(256), 0, s, qkv, cache, row_src, R, B, T, n_head, Tmax);
  COATI_LAUNCH_CHECK("kv_cache_fill_rows");
  return COATI_OK;
}

// out[b] = x[off[b + 1] - 1]: the last packed row of every sequence (f32 rows of C floats, R of them; a sequence of length 0 or one
// whose rows lie behind R -- a row count that did not match the lengths -- copies nothing)
__global__ __launch_bounds__(256) void gather_last_rows_kernel(const float* __restrict__ x, const int* __restrict__ off,
                                                               float* __restrict__ out, int B, int C, int R) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int last = off[b + 1] - 1;
  if (last < off[b] || last < 0 || last >= R) return;
  const float* src = x + (long long)last * C;
  for (int c = lane * 4; c < C; c += 256) *reinterpret_cast<float4*>(out + (long long)b * C + c) = *reinterpret_cast<const float4*>(src + c);
}
int launch_gather_last_rows(const float* x, const int* off, float* out, int B, int C, int R, hipStream_t s) {
  COATI_CHECK_ARG(x && off && out && C % 4 == 0, "gather_last_rows: null operand / C % 4");
  hipLaunchKernelGGL(gather_last_rows_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, x, off, out, B, C, R);
  COATI_LAUNCH_CHECK("gather_last_rows");
  return COATI_OK;
}
