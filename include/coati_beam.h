/*
 * coati_beam.h -- beam-search decoding over the KV-cached decode path of libcoati_hip.so (csrc/beam.hip, csrc/engine.cpp).
 *
 * A second header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), all pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a
 * hipStream_t passed as void*.  coati_hip.h and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart: it recomputes the whole prefix for every generated token and only samples
 * (smiles_xformer.py:272-351).
 *
 * Layout.  A decode session (coati_engine_decode_begin) of B = G * W rows serves G embeddings with W beams each; row g * W + r is beam
 * r of group g.  After every step the surviving beams are a permutation-with-repeats of the previous ones.  The cache rows do not
 * move: a record (row, t) is written once and never changes, so an ancestry table anc [B, Tmax] (int32) -- "position t of beam b
 * lives in cache row anc[b * Tmax + t]" -- is all the attention needs.  One step of the search:
 *
 *   coati_beam_row_topk   per row, its W best continuations by cum + log_softmax(logits)
 *   coati_beam_merge      per group, the best W of the W * W candidates become the new rows (scores, flags, ancestry, token history)
 *   coati_engine_decode_step_beams   the decode step on the new rows' tokens, attention through the new ancestry table
 */
#ifndef COATI_BEAM_H
#define COATI_BEAM_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* coati_attn_decode_hs with the record of position t < pos of row b read from cache row anc[b * Tmax + t] (int32 [B, Tmax]; an entry
 * outside 0 .. B - 1 reads row b).  The new (k, v) is still appended at (b, pos).  The arithmetic is coati_attn_decode_hs's, statement
 * for statement: with anc[b][t] = b the output is bit-identical.  head_size 16 or 32, Tmax <= 256. */
int coati_attn_decode_anc(const uint16_t* qkv, uint16_t* cache, uint16_t* y, int B, int n_head, int head_size, int Tmax, int pos,
                          const int32_t* anc, void* stream);

/* Per row b of logits [G * W, V] f32 (row stride ldl): cand_score / cand_tok [G * W, W] = the row's W largest logits as
 * (cum[b] + logit - lse(row), token), logit descending, token ascending.  A row with fin[b] != 0 emits (cum[b], pad_token) and W - 1
 * candidates of score -inf; a row with cum[b] == -inf emits -inf only (the first step starts each group from cum = [0, -inf, ...], so
 * that W identical rows yield the W distinct continuations of row 0).  1 <= W <= 16, W <= V, V * 4 <= 120 KiB. */
int coati_beam_row_topk(const float* logits, int64_t ldl, int G, int W, int V, const float* cum, const int32_t* fin, int pad_token,
                        float* cand_score, int32_t* cand_tok, void* stream);

/* Per group g: the best W of its W * W candidates (cand[(g * W + p) * W + j] comes from parent row g * W + p), by score descending,
 * then parent row ascending, then token ascending, become rows g * W + 0 .. W - 1 in rank order.  For new row r with parent p (a
 * global row index) and token tok:
 *   cum_out[r] = the score;  fin_out[r] = fin_in[p] || tok == stop_token;  len_out[r] = len_in[p] + (fin_in[p] ? 0 : 1);
 *   tok_next[r] = tok (int64: the next step's token vector);
 *   anc_out[r][0 .. pos-1] = anc_in[p][0 .. pos-1], anc_out[r][pos] = p   (pos = the position the last decode step appended at);
 *   hist_out[r][0 .. n-1] = hist_in[p][0 .. n-1],   hist_out[r][n] = tok   (int64 rows of stride ldh; n = beam steps taken so far).
 * nfin[g] = the group's finished rows.  Every *_in / *_out pair is a ping-pong pair of distinct buffers of the caller.
 * 1 <= W <= 16, 0 <= pos < Tmax, 0 <= n < ldh. */
int coati_beam_merge(const float* cand_score, const int32_t* cand_tok, int G, int W, const float* cum_in, const int32_t* fin_in,
                     const int32_t* len_in, const int32_t* anc_in, const int64_t* hist_in, int64_t ldh, int Tmax, int pos, int n,
                     int stop_token, float* cum_out, int32_t* fin_out, int32_t* len_out, int32_t* anc_out, int64_t* hist_out,
                     int64_t* tok_next, int32_t* nfin, void* stream);

/* coati_engine_decode_step on the session of coati_engine_decode_begin with every layer's attention in ancestry mode
 * (coati_attn_decode_anc on anc [B, Tmax] of the session's B and Tmax); advances the session's position.  Not captured into the
 * decode graphs.  Refused with a null anc and in a ragged session (coati_engine_decode_step_rows / _prefill_rows have run). */
int coati_engine_decode_step_beams(coati_engine* e, const int64_t* tokens, const int32_t* anc, const float* injection, float* logits,
                                   int64_t ldl, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_BEAM_H */
