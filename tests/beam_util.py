"""A pure-torch restatement of the beam search of include/coati_beam.h, in float64, for the tests: one group at a time, scores =
cum + log_softmax(logits) in float64, order = score descending, parent row ascending, token ascending, and the finished-row rule (a
finished hypothesis continues as itself with pad_token, its score and length unchanged)."""
import torch

NEG_INF = float("-inf")


def select(logits, cum, fin, W, pad_token):
    """One group's selection.  logits [R, V] (any float dtype; row p = parent p), cum [R] floats, fin [R] bools.  Returns
    (best, gap): best = the at most W candidates (score, parent, token) of finite score in rank order; gap = score of the last one kept
    minus the score of the first one left out (inf when nothing finite is left out, or fewer than W are kept)."""
    logp = torch.log_softmax(torch.as_tensor(logits).to(torch.float64), dim=-1)
    cand = []
    for p in range(logp.shape[0]):
        c = float(cum[p])
        if c == NEG_INF:
            continue
        if fin[p]:
            cand.append((c, p, int(pad_token)))
            continue
        sc = (c + logp[p]).tolist()
        cand += [(s, p, t) for t, s in enumerate(sc) if s != NEG_INF]
    cand.sort(key=lambda x: (-x[0], x[1], x[2]))
    best = cand[:W]
    gap = best[-1][0] - cand[W][0] if len(cand) > W and len(best) == W else float("inf")
    return best, gap


def merge(best, fin, length, stop_token):
    """(cum, fin, len) lists of the new rows from select()'s `best` and the parents' fin / len"""
    cum_o = [s for s, _, _ in best]
    fin_o = [bool(fin[p]) or t == int(stop_token) for _, p, t in best]
    len_o = [int(length[p]) + (0 if fin[p] else 1) for _, p, _ in best]
    return cum_o, fin_o, len_o


def beam_search(logits_fn, W, steps, stop_token, pad_token=0):
    """The search of one group from the empty continuation.  logits_fn(list of token lists) -> [n, V] logits of the next token behind
    each (the lists hold the generated tokens only; a prompt is logits_fn's business).  At most `steps` tokens; ends early when every
    hypothesis has finished.  Returns (hyps, trace): hyps = [(tokens, score, length, finished)] in rank order (tokens padded with
    pad_token behind [STOP], all of one length); trace = per step (best, gap) of select()."""
    toks, cum, fin, length = [[]], [0.0], [False], [0]
    trace = []
    for _ in range(steps):
        best, gap = select(logits_fn(toks), cum, fin, W, pad_token)
        trace.append((best, gap))
        toks = [toks[p] + [t] for _, p, t in best]
        cum, fin, length = merge(best, fin, length, stop_token)
        if all(fin):
            break
    return list(zip(toks, cum, length, fin)), trace
