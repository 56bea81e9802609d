/*
 * coati_grammar.h -- syntax-constrained decoding on the logits of libcoati_hip.so's decode paths (csrc/grammar.hip).
 *
 * A fourth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), all pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a
 * hipStream_t passed as void*.  coati_hip.h and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart: it samples, and checks the finished string with rdkit afterwards.
 *
 * The vocabulary's tokens are multi-symbol pieces of SMILES, so whether a token may follow is a matter of a per-row state and a
 * per-token transfer entry (coati_amd/grammar.py builds the entries and restates the rules in Python):
 *
 *   row state, int32 [B, 4]:   depth (open parentheses), rings (bit d: ring digit d is open, d = 0 .. 9),
 *                              flags (bit 0: inside a bracket atom, bit 1: dead, bit 2: finished), 0
 *   cost(s) = depth + popcount(rings) + (flags & 1): the single-symbol closers still owed
 *   entry, 8 bytes little-endian, table [2][V] indexed by (the bracket state the token is entered in, token):
 *     byte 0      need: the depth the token's prefix requires
 *     byte 1      delta: int8, net change of depth
 *     byte 2-3    toggle: the ring digits the token flips
 *     byte 4      bit 0: may be sampled from this state, bit 1: the bracket state at the token's end, bit 2: neutral (a special token)
 */
#ifndef COATI_GRAMMAR_H
#define COATI_GRAMMAR_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One launch per decode step, one workgroup per row b of logits [B, V] f32 (row stride ldl >= V).
 *
 * Advance: state_out[b] = state_in[parent ? parent[b] : b] advanced by tok_prev[b] (tok_prev == NULL: copied).  A finished or dead
 * state stays; stop_token finishes the row (dead if cost != 0); a neutral token or an id outside 0 .. V - 1 leaves the state alone; a
 * token that may not be sampled from the state or needs more depth makes the row dead; otherwise the state becomes
 * s' = (depth + delta, rings ^ toggle, the token's end bracket state), dead if cost(s') > remaining - 1.  parent (int32 [B], the beam
 * merge's parent row; an entry outside 0 .. B - 1 reads row b) needs state_in != state_out; without it they may be the same buffer.
 *
 * Mask: `remaining` counts the positions still to be drawn, the one these logits serve included.  In an alive, unfinished row
 * stop_token is admitted iff cost == 0, any other token iff it may be sampled from the row's bracket state, depth >= need and
 * cost(s') <= remaining - 2 (room for the closers and [STOP]).  -inf is stored into every entry that is not admitted, and only there:
 * the logits are not read, admitted entries and the columns V .. ldl - 1 are not written.  A dead or finished row is left untouched. */
int coati_grammar_step(float* logits, int64_t ldl, int B, int V, const uint64_t* table, const int32_t* state_in, int32_t* state_out,
                       const int64_t* tok_prev, const int32_t* parent, int remaining, int stop_token, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_GRAMMAR_H */
