// Syntax-constrained decoding (include/coati_grammar.h): per decode step one launch that advances every row's automaton state by the
// token it drew and stores -inf over the logits of the tokens that may not follow.  The rules, with their commentary, are restated in
// Python in coati_amd/grammar.py; the header describes the state and the table entry.
//
// A streaming kernel over the row's V 8-byte entries ([2][V], shared by all rows, cache-resident): the mask does not depend on the
// logits, so they are not read -- a lane loads four entries with two 16-byte loads and issues at most four predicated dword stores.
#include "../../include/coati_grammar.h"
#include "kernels.h"

#define GR_INBR 1
#define GR_DEAD 2
#define GR_FIN 4
#define GE_SAMP 1
#define GE_ENDBR 2
#define GE_NEUTRAL 4

__device__ __forceinline__ int gr_need(unsigned long long e) { return (int)(e & 0xffu); }
__device__ __forceinline__ int gr_delta(unsigned long long e) { return (int)(signed char)((e >> 8) & 0xffu); }
__device__ __forceinline__ int gr_toggle(unsigned long long e) { return (int)((e >> 16) & 0xffffu); }
__device__ __forceinline__ int gr_flags(unsigned long long e) { return (int)((e >> 32) & 0xffu); }

// the token of entry e (of the row's bracket state) may be drawn: sampleable, its prefix fits the depth, cost(s') within the budget
__device__ __forceinline__ bool gr_admit(unsigned long long e, int depth, int rings, int budget) {
  const int fl = gr_flags(e);
  const int cost = depth + gr_delta(e) + __popc((unsigned)(rings ^ gr_toggle(e))) + ((fl & GE_ENDBR) ? 1 : 0);
  return (fl & GE_SAMP) && depth >= gr_need(e) && cost <= budget;
}

__global__ __launch_bounds__(256) void grammar_step_kernel(float* __restrict__ logits, long long ldl, int B, int V,
                                                           const unsigned long long* __restrict__ table, const int* state_in,
                                                           int* state_out, const long long* __restrict__ tok_prev,
                                                           const int* __restrict__ parent, int remaining, int stop_token) {
  __shared__ int s_st[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  // thread 0 alone reads the old state and writes the new one: state_in may be state_out (without parent)
  if (tid == 0) {
    int src = b;
    if (parent) {
      const int p = parent[b];
      src = (p >= 0 && p < B) ? p : b;
    }
    int depth = state_in[4 * (long long)src], rings = state_in[4 * (long long)src + 1], flags = state_in[4 * (long long)src + 2];
    if (tok_prev && !(flags & (GR_DEAD | GR_FIN))) {
      const long long t = tok_prev[b];
      const int inbr = flags & GR_INBR;
      if (t == stop_token) {
        flags |= GR_FIN | ((depth + __popc((unsigned)rings) + inbr) != 0 ? GR_DEAD : 0);
      } else if (t >= 0 && t < V) {
        const unsigned long long e = table[(long long)inbr * V + t];
        const int fl = gr_flags(e);
        if (fl & GE_NEUTRAL) {
        } else if (!(fl & GE_SAMP) || depth < gr_need(e)) {
          flags |= GR_DEAD;
        } else {
          depth += gr_delta(e);
          rings ^= gr_toggle(e);
          const int br = (fl & GE_ENDBR) ? 1 : 0;
          flags = (flags & ~GR_INBR) | br;
          if (depth + __popc((unsigned)rings) + br > remaining - 1) flags |= GR_DEAD;
        }
      }
    }
    s_st[0] = depth;
    s_st[1] = rings;
    s_st[2] = flags;
    int* so = state_out + 4 * (long long)b;
    so[0] = depth;
    so[1] = rings;
    so[2] = flags;
    so[3] = 0;
  }
  __syncthreads();
  const int depth = s_st[0], rings = s_st[1], flags = s_st[2];
  if (flags & (GR_DEAD | GR_FIN)) return;
  const int inbr = flags & GR_INBR;
  const bool stop_ok = depth + __popc((unsigned)rings) + inbr == 0;
  const int budget = remaining - 2;
  float* lrow = logits + (long long)b * ldl;
  const unsigned long long* trow = table + (long long)inbr * V;
  // where the table's row starts 8 bytes off a 16-byte boundary (V odd, second row), one entry goes ahead of the 16-byte loads
  int head = (int)((reinterpret_cast<unsigned long long>(trow) >> 3) & 1ull);
  head = head < V ? head : V;
  const int quads = (V - head) >> 2;
  const ulonglong2* tq = reinterpret_cast<const ulonglong2*>(trow + head);
  for (int q = tid; q < quads; q += 256) {
    const ulonglong2 e01 = tq[2 * q], e23 = tq[2 * q + 1];
    const int i = head + 4 * q;
    const bool a0 = (i == stop_token) ? stop_ok : gr_admit(e01.x, depth, rings, budget);
    const bool a1 = (i + 1 == stop_token) ? stop_ok : gr_admit(e01.y, depth, rings, budget);
    const bool a2 = (i + 2 == stop_token) ? stop_ok : gr_admit(e23.x, depth, rings, budget);
    const bool a3 = (i + 3 == stop_token) ? stop_ok : gr_admit(e23.y, depth, rings, budget);
    if (!a0) lrow[i] = -INFINITY;
    if (!a1) lrow[i + 1] = -INFINITY;
    if (!a2) lrow[i + 2] = -INFINITY;
    if (!a3) lrow[i + 3] = -INFINITY;
  }
  // scalar head and tail: entry 0 when head == 1, and the V - head - 4 * quads < 4 entries behind the last quad
  const int tail0 = head + 4 * quads;
  if (tid < head + (V - tail0)) {
    const int i = tid < head ? 0 : tail0 + (tid - head);
    const bool a = (i == stop_token) ? stop_ok : gr_admit(trow[i], depth, rings, budget);
    if (!a) lrow[i] = -INFINITY;
  }
}

int coati_grammar_step(float* logits, int64_t ldl, int B, int V, const uint64_t* table, const int32_t* state_in, int32_t* state_out,
                       const int64_t* tok_prev, const int32_t* parent, int remaining, int stop_token, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(logits && table && state_in && state_out, "grammar_step: null operand");
  COATI_CHECK_ARG(parent == nullptr || state_in != state_out, "grammar_step: with parent, state_in and state_out must differ (ping-pong)");
  COATI_CHECK_ARG((reinterpret_cast<unsigned long long>(table) & 7ull) == 0, "grammar_step: the table must start at an 8-byte boundary");
  COATI_CHECK_SHAPE(B >= 1 && V >= 1 && ldl >= V && remaining >= 1 && stop_token >= 0 && stop_token < V,
                    "grammar_step: unsupported shape B=%d V=%d ldl=%lld remaining=%d stop_token=%d (ldl >= V, remaining >= 1, 0 <= stop_token < V)",
                    B, V, (long long)ldl, remaining, stop_token);
  hipLaunchKernelGGL(grammar_step_kernel, dim3(B), dim3(256), 0, s, logits, ldl, B, V, reinterpret_cast<const unsigned long long*>(table), state_in,
                     state_out, LL(tok_prev), parent, remaining, stop_token);
  COATI_LAUNCH_CHECK("grammar_step");
  return COATI_OK;
}
