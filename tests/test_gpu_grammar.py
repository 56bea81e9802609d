"""Syntax-constrained decoding on the GPU (include/coati_grammar.h, coati_amd/grammar.py): coati_grammar_step against the Python
restatement element for element, the sampler's fallback on rows with fewer than k finite logits, and grammar= on the engine's sampling,
prompt-completion and beam-search paths with the real `may_closedparen` vocabulary slice (V = 2697) on a small random-weight engine."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import beam_util  # noqa: E402
from tests import grammar_util as U  # noqa: E402
from tests.gpu_util import log  # noqa: E402

DEV = "cuda:0"
V, N_SEQ = 2697, 24
SMALL = dict(n_layer_e3gnn=1, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=N_SEQ, n_tok=V)
PREFIX = [8, 7, 2]                                # [CLIP][UNK][SMILES]
STOP, PAD, UNK = 1, 0, 7
NEG = float("-inf")
DEAD, FINISHED = 2, 4


def _sample(logits, k, u, inv_temp=1.0):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.long, device=DEV)
    _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, V, int(k), float(inv_temp), ptr(u), ptr(out), None, STOP, PAD, stream())
    return out.cpu()


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
_KERNEL = {}


def _kernel_inputs():
    """shared, never written: 64 states (alive, dead, finished), logits [64, V + 3], forced tokens of every kind, a parent map"""
    if not _KERNEL:
        gr = U.grammar()
        rng = np.random.default_rng(5)
        states = U.random_states(64, seed=11)
        kinds = [bool(s[2] & DEAD) for s in states], [bool(s[2] & FINISHED) for s in states]
        assert 4 <= sum(kinds[0]) <= 40 and sum(kinds[1]) >= 4 and sum(1 for s in states if s[2] & 1) >= 1, states
        tok = []
        for b, s in enumerate(states):          # admitted tokens, any SMILES token, [STOP], a special token, an id outside the vocabulary
            if b % 8 < 4:
                tok.append(int(rng.choice(np.flatnonzero(gr.admitted(s, 10)))))
            elif b % 8 < 6:
                tok.append(int(rng.integers(320, V)))
            else:
                tok.append([STOP, PAD, V + 5, -1][(b // 8) % 4])
        _KERNEL.update(states=states, tok=tok, parent=[int(p) for p in rng.integers(0, 64, 64)],
                       logits=torch.randn(64, V + 3, generator=torch.Generator().manual_seed(6)))
    return _KERNEL


@pytest.mark.parametrize("mode", ["copy", "tok_prev", "tok_prev_in_place", "parent"])
@pytest.mark.parametrize("remaining", [1, 2, 3, 10])
def test_grammar_step_equals_the_restatement(remaining, mode):
    gr, k = U.grammar(), _kernel_inputs()
    states, B = k["states"], 64
    tok = k["tok"] if mode != "copy" else None
    parent = k["parent"] if mode == "parent" else None
    want_state, want_mask = [], np.ones((B, V + 3), dtype=bool)
    for b in range(B):
        s = states[parent[b] if parent else b]
        if tok is not None:
            s = gr.advance(s, tok[b], remaining)
        want_state.append([s[0], s[1], s[2], 0])
        want_mask[b, :V] = gr.admitted(s, remaining)
    logits = k["logits"].to(DEV)
    s_in = gr.states(states, DEV)
    s_out = s_in if mode == "tok_prev_in_place" else torch.full_like(s_in, -7)
    gr.step(logits, s_in, s_out, tok_prev=None if tok is None else torch.tensor(tok, dtype=torch.long, device=DEV),
            parent=None if parent is None else torch.tensor(parent, dtype=torch.int32, device=DEV), remaining=remaining)
    torch.cuda.synchronize()
    assert s_out.cpu().tolist() == want_state
    if mode != "tok_prev_in_place":
        assert s_in.cpu().tolist() == [[s[0], s[1], s[2], 0] for s in states]
    want = torch.where(torch.from_numpy(want_mask), k["logits"], torch.full_like(k["logits"], NEG))
    assert torch.equal(_bits(logits.cpu()), _bits(want))                     # masked entries -inf, all others (the 3 columns past V too) untouched
    from coati_amd.grammar import cost
    alive = [not (w[2] & (DEAD | FINISHED)) for w in want_state]
    n_adm = [int(want_mask[b, :V].sum()) for b in range(B) if alive[b]]
    # never empty where the invariant cost <= R - 1 holds (the walks behind these states had no length budget: some owe more)
    assert all(want_mask[b, :V].any() for b in range(B) if alive[b] and cost(tuple(want_state[b][:3])) <= remaining - 1)
    log(f"grammar_step R={remaining} {mode}: {sum(alive)}/64 rows constrained, admitted {min(n_adm)} .. {max(n_adm)} of {V}")


# ---- 2. the sampler's fallback --------------------------------------------------------------------------------------------------------
def test_sampler_falls_back_to_the_last_candidate_of_non_zero_weight():
    """rows with exactly one finite logit: with u = 1.0 the running sum never exceeds u * z, and the fallback must be that token, not
    candidate k - 1 (a -inf entry)"""
    where = [0, 1, 1348, V - 1]
    logits = torch.full((4, V), NEG)
    for b, t in enumerate(where):
        logits[b, t] = [0.5, -3.0, 40.0, -1e30][b]
    logits = logits.to(DEV)
    assert _sample(logits, 100, torch.ones(4, device=DEV)).tolist() == where
    assert _sample(logits, 100, torch.full((4,), 0.999999, device=DEV)).tolist() == where
    assert _sample(logits, 1, torch.ones(4, device=DEV)).tolist() == where
    assert _sample(logits, 1, torch.zeros(4, device=DEV)).tolist() == where
    two = torch.full((2, V), NEG)                 # two finite logits: u = 1.0 falls back to the smaller one, never to a -inf entry
    two[:, 7], two[:, 2000] = 1.0, 0.0
    assert _sample(two.to(DEV), 100, torch.ones(2, device=DEV)).tolist() == [2000, 2000]


# ---- 3. the mask in front of the existing sampler ---------------------------------------------------------------------------------------
def test_grammar_step_then_sampler_equals_the_sampler_on_torch_masked_logits():
    gr, k = U.grammar(), _kernel_inputs()
    states = k["states"]
    base = k["logits"][:, :V].contiguous()
    u = torch.rand(64, generator=torch.Generator().manual_seed(8)).to(DEV)
    for remaining in (3, 10):
        mask = torch.from_numpy(np.stack([gr.admitted(s, remaining) for s in states]))
        masked = torch.where(mask, base, torch.full_like(base, NEG)).to(DEV)
        logits = base.to(DEV)
        s = gr.states(states, DEV)
        gr.step(logits, s, s, remaining=remaining)
        got, want = _sample(logits, 100, u), _sample(masked, 100, u)
        assert got.tolist() == want.tolist()
        # only admitted tokens are drawn (R = 3 leaves some of these states, walked without a length budget, with none)
        assert all(bool(mask[b, t]) for b, t in enumerate(got.tolist()) if bool(mask[b].any()))
        assert remaining != 10 or bool(mask.any(1).all())


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
_ENGINE = {}


def _engine():
    if not _ENGINE:
        from coati_amd.engine import Engine, ModelConfig
        eng = Engine(ModelConfig(**SMALL), DEV, train=False)
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for name, (off, shape) in eng.layout.items():
                v = eng.view(name)
                if len(shape) == 2:
                    v.copy_((torch.randn(shape, generator=g) * (0.1 if "tok_emb" not in name else 1.0)).to(DEV))
                elif name.endswith("weight"):
                    v.fill_(1.0)
            head = [k for k in eng.layout if "lm_head" in k][0]
            eng.view(head)[STOP] *= 2.5                   # random weights hardly ever stop: rows and beams should also end early
        eng.refresh_shadows()
        _ENGINE["eng"] = eng
        _ENGINE["payload"] = torch.randn(64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    return _ENGINE["eng"], _ENGINE["payload"]


def _generate(eng, payload, grammar, seed, k=100):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = eng.generate_top_k_with_inj_batch(prefix=PREFIX, stop_token=STOP, pad_token=PAD, inv_temp=1.0, k=k, inj_token=UNK,
                                             inj_payload=payload, generator=g, grammar=grammar)
    return rows, eng.last_unstopped.cpu().tolist(), None if grammar is None else eng.last_grammar_violations.cpu().tolist()


# ---- 4. a table that admits everything changes nothing ------------------------------------------------------------------------------------
def test_all_permissive_table_draws_the_same_tokens():
    """every token sampleable with need 0, delta 0, toggle 0 (the special tokens too: a random-weight model draws them, and the plain
    path does not exclude them), so cost stays 0 and [STOP] is always admitted.  Only the last position differs in the making: the
    grammar admits [STOP] alone there, the plain path overwrites it with [STOP] -- the returned rows are the same, bit for bit."""
    from coati_amd.grammar import SmilesGrammar
    eng, payload = _engine()
    z = np.zeros((2, V), dtype=np.int64)
    free = SmilesGrammar(z, z, z, z + 1, STOP)
    plain, unstopped, _ = _generate(eng, payload, None, seed=3)
    got, unstopped_g, viol = _generate(eng, payload, free, seed=3)
    assert got == plain and len(got) == 64 and len(got[0]) == N_SEQ
    assert not any(unstopped_g) and not any(viol)
    log(f"all-permissive grammar: 64 rows equal; plain path overwrote the last position of {sum(unstopped)} rows")


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------------
SEED = 3          # the first seed tried; the plain run leaves unbalanced rows with it (see the log line)


def test_every_constrained_row_is_balanced_and_stops_on_its_own():
    from coati_amd.grammar import balanced
    eng, payload = _engine()
    gr = U.grammar()
    rows, unstopped, viol = _generate(eng, payload, gr, SEED)
    assert len(rows) == 64 and all(r[:3] == PREFIX for r in rows)
    bad = [U.text(r[3:]) for r in rows if not balanced(U.text(r[3:]))]
    assert not bad, bad
    assert not any(unstopped), unstopped                                  # every row drew its [STOP] before the overwrite
    assert not any(viol), viol
    assert all(STOP in r[3:] for r in rows)
    assert all(t >= 320 or t in (STOP, PAD) for r in rows for t in r[3:])       # no special token is drawn
    lens = [r[3:].index(STOP) + 1 for r in rows]
    plain, unstopped_p, _ = _generate(eng, payload, None, SEED)
    n_bad = sum(not balanced(U.text(r[3:])) for r in plain)
    log(f"constrained sampling, seed {SEED}: 64/64 balanced, lengths {min(lens)} .. {max(lens)}, 0 rows overwritten; "
        f"plain: {n_bad}/64 unbalanced, {sum(unstopped_p)}/64 rows overwritten with [STOP]")
    assert n_bad >= 1


# ---- 6. prompt completion ---------------------------------------------------------------------------------------------------------------------
def test_prompts_advance_the_state_and_broken_prompts_are_flagged():
    from coati_amd.grammar import balanced
    eng, _ = _engine()
    gr, tk = U.grammar(), U.tokenizer()
    prompts = [tk.tokenize_text("[SMILES]c1ccc(", pad=False), tk.tokenize_text("[SMILES]CC(=O)N[", pad=False), [2, tk.vocab[")"]]]
    assert len({len(p) for p in prompts}) == 3
    assert gr.walk(prompts[0])[:2] == (1, 2) and gr.walk(prompts[1]) == (0, 0, 1)
    g = torch.Generator(device=DEV).manual_seed(4)
    out = eng.generate_topk_batch(prompts, STOP, PAD, inv_temp=1.0, k=100, generator=g, grammar=gr)
    viol = eng.last_grammar_violations.cpu().tolist()
    assert viol == [False, False, True]
    for p, row in zip(prompts, out):
        assert row[:len(p)] == p and len(row) == N_SEQ
    for row in out[:2]:
        assert STOP in row and balanced(U.text(row)), U.text(row)
        assert all(t >= 320 for t in row[1:row.index(STOP)])
    # the other rows do not depend on the broken one: the same call without it draws the same tokens (the uniforms are per row)
    g = torch.Generator(device=DEV).manual_seed(4)
    again = eng.generate_topk_batch(prompts[:2] + [[2, tk.vocab["C"]]], STOP, PAD, inv_temp=1.0, k=100, generator=g, grammar=gr)
    assert again[:2] == out[:2] and eng.last_grammar_violations.cpu().tolist() == [False, False, False]
    assert balanced(U.text(again[2]))
    one = eng.generate_topk_with_inj(prompts[0], STOP, inv_temp=1.0, k=100, generator=torch.Generator(device=DEV).manual_seed(5), grammar=gr)
    assert one[-1] == STOP and balanced(U.text(one)) and eng.last_grammar_violations.cpu().tolist() == [False]
    log(f"completions: {U.text(out[0])!r}, {U.text(out[1])!r}; broken prompt row: {U.text(out[2])!r}")


# ---- 7. beam search -------------------------------------------------------------------------------------------------------------------------------
def test_beam_search_under_the_grammar_matches_the_restatement():
    """beam_util's selection in float64 on the log-softmax of the masked logits, the logits being those of teacher-forced plain decode
    steps of the same engine (the bits the search sees).  Scores within 1e-4 x length and parents / tokens equal step by step while the
    restatement's W-th and (W+1)-th candidates are further apart than that, as in tests/test_gpu_beam.py; at least three quarters of the
    groups must compare to their end."""
    from coati_amd.grammar import balanced
    eng, payload = _engine()
    gr = U.grammar()
    G, W, m = 8, 4, len(PREFIX)
    steps = N_SEQ - m
    pay = payload[:G].contiguous()
    trace = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = eng._beam_search(PREFIX, STOP, PAD, W, UNK, pay, None, 0.0, trace=trace, grammar=gr)
    torch.cuda.current_stream().wait_stream(side)
    viol = eng.last_grammar_violations.cpu()
    tokens, scores, lengths, finished = (x.cpu() for x in out)
    trace = [tuple(x.cpu() for x in step) for step in trace]
    again = eng.beam_search(PREFIX, STOP, PAD, beams=W, inj_token=UNK, inj_payload=pay, grammar=gr)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again, (tokens, scores, lengths, finished)))
    assert viol.shape == (G, W) and not bool(viol.any())
    n_finite = 0
    for g in range(G):
        for r in range(W):
            if float(scores[g, r]) == NEG:
                continue
            n_finite += 1
            gen = tokens[g, r, m:].tolist()
            assert bool(finished[g, r]) and gen[int(lengths[g, r]) - 1] == STOP and balanced(U.text(gen)), (g, r, gen)
    assert n_finite >= G * W - G

    def masked_logits(hyps):
        """[n, V] float64: the masked logits behind PREFIX + hyp for every hypothesis, one teacher-forced session for all of them"""
        n, length = len(hyps), len(hyps[0][1])
        rows = torch.tensor([PREFIX + h for _, h in hyps], dtype=torch.long, device=DEV)
        inj = torch.stack([pay[g] for g, _ in hyps])
        eng.decode_begin(n, N_SEQ)
        for t in range(m + length):
            lg = eng.decode_step(rows[:, t].contiguous(), inj if t == 1 else None, want_logits=(t == m + length - 1))
        lg = lg.double().cpu()
        for i, (_, h) in enumerate(hyps):
            adm = torch.from_numpy(gr.admitted(gr.walk(PREFIX + h, N_SEQ), steps - length))
            lg[i, ~adm] = NEG
        return lg

    # the groups in lockstep: per group the restatement's (tokens, cum, fin, len) lists
    state = [dict(toks=[[]], cum=[0.0], fin=[False], len=[0], clear=True, done=False) for _ in range(G)]
    compared = 0
    for s in range(len(trace)):
        live = [(g, t) for g in range(G) if not state[g]["done"] for t in state[g]["toks"]]
        if not live:
            break
        width = max(len(t) for _, t in live)
        assert all(len(t) == width for _, t in live)
        lg = masked_logits(live)
        at = 0
        for g in range(G):
            st = state[g]
            if st["done"]:
                continue
            n = len(st["toks"])
            best, gap = beam_util.select(lg[at:at + n], st["cum"], st["fin"], W, PAD)
            at += n
            st["clear"] = st["clear"] and gap >= 1e-4
            if st["clear"]:
                got = [(int(trace[s][0][g * W + r]) - g * W, int(trace[s][1][g * W + r])) for r in range(len(best))]
                assert got == [(p, t) for _, p, t in best], (g, s, got, best, gap)
                sc = trace[s][2][g * W:g * W + len(best)].double()
                err = (sc - torch.tensor([b[0] for b in best], dtype=torch.float64)).abs().max()
                assert float(err) <= 1e-4 * (s + 1), (g, s, float(err))
                compared += 1
            st["toks"] = [st["toks"][p] + [t] for _, p, t in best]
            st["cum"], st["fin"], st["len"] = beam_util.merge(best, st["fin"], st["len"], STOP)
            st["done"] = all(st["fin"])
    to_end = sum(st["clear"] for st in state)
    log(f"beam search under the grammar: {n_finite}/{G * W} hypotheses finite, all balanced and finished; {to_end}/{G} groups equal the "
        f"restatement to their end ({compared} group-steps compared), lengths {int(lengths.min())} .. {int(lengths.max())}")
    assert to_end >= 0.75 * G, to_end


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_paths_that_do_not_take_a_grammar_refuse_it():
    eng, payload = _engine()
    gr = U.grammar()
    with pytest.raises(NotImplementedError, match="ragged"):
        eng.generate_topk_batch([[2, 400], [2, 401, 402]], STOP, PAD, ragged=True, grammar=gr)
    with pytest.raises(NotImplementedError, match="slots"):
        eng.generate_stream(PREFIX, STOP, PAD, inj_token=UNK, inj_payload=payload[:4], slots=2, grammar=gr)
    with pytest.raises(NotImplementedError, match="use_graph"):
        eng.generate_top_k_with_inj_batch(prefix=PREFIX, stop_token=STOP, pad_token=PAD, inj_token=UNK, inj_payload=payload[:4],
                                          use_graph=True, grammar=gr)
    from coati_amd.grammar import SmilesGrammar
    z = np.zeros((2, 48), dtype=np.int64)
    with pytest.raises(ValueError, match="built for 48 tokens"):
        eng.generate_top_k_with_inj_batch(prefix=PREFIX, stop_token=STOP, pad_token=PAD, inj_token=UNK, inj_payload=payload[:4],
                                          grammar=SmilesGrammar(z, z, z, z + 1, STOP))
