"""Beam search over the KV-cached decode path (include/coati_beam.h): the ancestry-following attention against the plain one on a
physically gathered cache, the selection kernels against the float64 restatement (tests/beam_util.py), and Engine.beam_search end to end:
against greedy decoding, against teacher-forced decode steps, against Engine.score and against the restatement on full-prefix logits."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import beam_util  # noqa: E402
from tests.gpu_util import log  # noqa: E402

DEV = "cuda:0"
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4,
             n_seq=24, n_tok=48)
HS32 = dict(SMALL, n_head=2)                      # head size 32
PREFIX = [8, 7, 2]                                # [CLIP][UNK][SMILES]
STOP, PAD, UNK = 1, 0, 7
TOL = 7e-3      # decode vs full pass, relative to the logit scale: the bound of tests/test_gpu_decode.py
INF = float("inf")


def _call(name, *args):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    _lib.call(name, *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], stream())


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV).contiguous()


# ---- 1. the attention --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 63, 64, 127, 128, 199])
@pytest.mark.parametrize("hs", [16, 32])
def test_attn_decode_anc_follows_the_ancestry_bit_for_bit(hs, pos):
    """B * n_head = 18 waves (not a multiple of the 4 per workgroup), positions at the 64-lane pass boundaries.  (a) identity table:
    y and the cache are coati_attn_decode_hs's bits; (b) a random within-group ancestry: y is coati_attn_decode_hs's on a cache that
    torch gathered by that ancestry; (c) only record (b, pos) of the cache changed."""
    B, W, nh, Tmax = 6, 3, 3, 200
    C = nh * hs
    g = torch.Generator().manual_seed(1000 * hs + pos)
    qkv = torch.randn(B, 3 * C, generator=g).bfloat16().to(DEV)
    cache0 = torch.randn(B, nh, Tmax, 2 * hs, generator=g).bfloat16().to(DEV)

    def run(name, cache, *anc):
        y = torch.zeros(B, C, dtype=torch.bfloat16, device=DEV)
        c = cache.clone()
        _call(name, qkv, c, y, B, nh, hs, Tmax, pos, *anc)
        return y.view(torch.int16), c.view(torch.int16)

    y_ref, c_ref = run("coati_attn_decode_hs", cache0)
    ident = _i32(torch.arange(B).view(B, 1).repeat(1, Tmax))
    y_id, c_id = run("coati_attn_decode_anc", cache0, ident)
    assert torch.equal(y_id, y_ref) and torch.equal(c_id, c_ref)
    anc = torch.arange(B).view(B, 1) // W * W + torch.randint(0, W, (B, Tmax), generator=g)
    rows = anc.to(DEV).view(B, 1, Tmax).expand(B, nh, Tmax)
    gathered = cache0[rows, torch.arange(nh, device=DEV).view(1, nh, 1), torch.arange(Tmax, device=DEV).view(1, 1, Tmax)].contiguous()
    y_gat, _ = run("coati_attn_decode_hs", gathered)
    y_anc, c_anc = run("coati_attn_decode_anc", cache0, _i32(anc))
    assert torch.equal(y_anc, y_gat)
    if pos > 0:
        assert not torch.equal(y_anc, y_ref)                         # (the ancestry does matter on these inputs)
    want = cache0.clone()
    want[:, :, pos, :hs] = qkv[:, C:2 * C].view(B, nh, hs)
    want[:, :, pos, hs:] = qkv[:, 2 * C:].view(B, nh, hs)
    assert torch.equal(c_anc, want.view(torch.int16))


# ---- 2. the selection kernels ------------------------------------------------------------------------------------------------------
# seeds at which, in the float64 restatement, every two adjacent scores among a group's first W + 1 candidates differ by more than 1e-3
SEL_SEEDS = {(1, 48): 0, (4, 48): 0, (16, 48): 0, (1, 10322): 0, (4, 10322): 0, (16, 10322): 0}
SEL_G, SEL_TMAX, SEL_POS, SEL_N, SEL_LDH = 3, 40, 17, 7, 12


def selection_case(W, V, seed):
    """host tensors of one selection problem: logits of scale 10 in rows of a padded stride (the padding holds 1e30: read, it would win),
    cum in [-60, 0], a third of the rows finished, random lengths, ancestry and token history"""
    g = torch.Generator().manual_seed(seed)
    G = SEL_G
    B = G * W
    ldl = (V + 7) // 8 * 8 + 8
    logits = torch.full((B, ldl), 1e30)
    logits[:, :V] = 10 * torch.randn(B, V, generator=g)
    return dict(W=W, V=V, G=G, logits=logits, cum=-60 * torch.rand(B, generator=g), fin=(torch.arange(B) % 3 == 1).to(torch.int32),
                len=torch.randint(1, 10, (B,), generator=g, dtype=torch.int32),
                anc=(torch.arange(B).view(B, 1) // W * W + torch.randint(0, W, (B, SEL_TMAX), generator=g)).to(torch.int32),
                hist=torch.randint(0, V, (B, SEL_LDH), generator=g))


def selection_restated(case, W=None):
    """per group (best, gap) of beam_util.select on the case (W: another beam count than the case's, for the margins)"""
    Wc, V = case["W"], case["V"]
    out = []
    for g in range(case["G"]):
        r = slice(g * Wc, (g + 1) * Wc)
        out.append(beam_util.select(case["logits"][r, :V], case["cum"][r].tolist(), case["fin"][r].tolist(), W or Wc, PAD))
    return out


def selection_margin(case):
    """the smallest difference of two adjacent scores among any group's first W + 1 candidates"""
    worst = INF
    for best, _ in selection_restated(case, case["W"] + 1):
        sc = [s for s, _, _ in best]
        worst = min([worst] + [a - b for a, b in zip(sc, sc[1:])])
    return worst


def run_selection(case, pos=SEL_POS, n=SEL_N):
    W, V, G = case["W"], case["V"], case["G"]
    B = G * W
    d = {k: v.to(DEV).contiguous() for k, v in case.items() if isinstance(v, torch.Tensor)}
    cand_s = torch.empty(B, W, device=DEV)
    cand_t = torch.empty(B, W, dtype=torch.int32, device=DEV)
    _call("coati_beam_row_topk", d["logits"], d["logits"].stride(0), G, W, V, d["cum"], d["fin"], PAD, cand_s, cand_t)
    out = dict(cum=torch.empty(B, device=DEV), fin=torch.empty(B, dtype=torch.int32, device=DEV), len=torch.empty(B, dtype=torch.int32, device=DEV),
               anc=torch.full_like(d["anc"], -7), hist=torch.full_like(d["hist"], -7), tok=torch.empty(B, dtype=torch.long, device=DEV),
               nfin=torch.empty(G, dtype=torch.int32, device=DEV))
    _call("coati_beam_merge", cand_s, cand_t, G, W, d["cum"], d["fin"], d["len"], d["anc"], d["hist"], d["hist"].stride(0), d["anc"].shape[1],
          pos, n, STOP, out["cum"], out["fin"], out["len"], out["anc"], out["hist"], out["tok"], out["nfin"])
    return {k: v.cpu() for k, v in out.items()}, cand_s.cpu(), cand_t.cpu()


def check_selection(case, out, pos=SEL_POS, n=SEL_N, tol=1e-4):
    """every output of the merge against the restatement: (parent, token) per rank exactly, scores within tol"""
    W = case["W"]
    worst = 0.0
    for g, (best, _) in enumerate(selection_restated(case)):
        assert len(best) == W
        cum, fin, length = beam_util.merge(best, case["fin"][g * W:(g + 1) * W].tolist(), case["len"][g * W:(g + 1) * W].tolist(), STOP)
        for r, (score, p, tok) in enumerate(best):
            row, parent = g * W + r, g * W + p
            assert (int(out["anc"][row, pos]), int(out["tok"][row])) == (parent, tok), (g, r)
            worst = max(worst, abs(float(out["cum"][row]) - score))
            assert bool(out["fin"][row]) == fin[r] and int(out["len"][row]) == length[r], (g, r)
            assert torch.equal(out["anc"][row, :pos], case["anc"][parent, :pos]) and bool((out["anc"][row, pos + 1:] == -7).all())
            assert torch.equal(out["hist"][row, :n], case["hist"][parent, :n]) and int(out["hist"][row, n]) == tok
            assert bool((out["hist"][row, n + 1:] == -7).all())
        assert int(out["nfin"][g]) == sum(fin)
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("V", [48, 10322])
@pytest.mark.parametrize("W", [1, 4, 16])
def test_selection_matches_the_float64_restatement(W, V):
    """scores within 1e-4: a handful of f32 roundings at magnitude <= 128 (one ulp 1.5e-5) with accurate expf / logf"""
    case = selection_case(W, V, SEL_SEEDS[(W, V)])
    margin = selection_margin(case)
    assert margin > 1e-3, f"seed {SEL_SEEDS[(W, V)]}: adjacent scores {margin:.2e} apart -- pick another seed"
    out, _, _ = run_selection(case)
    worst = check_selection(case, out)
    log(f"beam selection W={W} V={V}: margin {margin:.2e}, worst score error {worst:.2e}")


def test_selection_first_step_ties_and_finished_groups():
    V = 48
    g = torch.Generator().manual_seed(3)
    # the first step: W identical rows, cum = [0, -inf, ...] -> the W best continuations of row 0, all with parent row 0 of the group
    case = selection_case(4, V, 11)
    case["logits"][:, :V] = case["logits"][::4, :V].repeat_interleave(4, dim=0)
    case["cum"] = torch.tensor([0.0, -INF, -INF, -INF]).repeat(case["G"])
    case["fin"] = torch.zeros(12, dtype=torch.int32)
    case["len"] = torch.zeros(12, dtype=torch.int32)
    out, cand_s, _ = run_selection(case, pos=2, n=0)
    check_selection(case, out, pos=2, n=0)
    for grp in range(case["G"]):
        top = torch.topk(case["logits"][4 * grp, :V], 4)
        assert out["tok"][4 * grp:4 * grp + 4].tolist() == top.indices.tolist() and len(set(top.indices.tolist())) == 4
        assert out["anc"][4 * grp:4 * grp + 4, 2].tolist() == [4 * grp] * 4
        assert bool((cand_s[4 * grp + 1:4 * grp + 4] == -INF).all())
    # exact ties: rows 0 and 1 identical with equal cum, and two equal logits (tokens 5 and 9) at their top
    case = selection_case(4, V, 12)
    case["G"] = 1
    for k in ("logits", "cum", "fin", "len", "anc", "hist"):
        case[k] = case[k][:4].clone()
    case["logits"][0, :V] = torch.randn(V, generator=g)
    case["logits"][0, 5] = case["logits"][0, 9] = 9.0
    case["logits"][1] = case["logits"][0]
    case["cum"] = torch.tensor([-1.0, -1.0, -30.0, -30.0])
    case["fin"] = torch.zeros(4, dtype=torch.int32)
    case["anc"] = case["anc"] % 4
    out, _, _ = run_selection(case)
    check_selection(case, out)
    assert list(zip(out["anc"][:, SEL_POS].tolist(), out["tok"].tolist())) == [(0, 5), (0, 9), (1, 5), (1, 9)]
    assert out["cum"][0] == out["cum"][1] == out["cum"][2] == out["cum"][3]
    # a group whose rows are all finished reproduces itself
    case = selection_case(3, V, 13)
    case["fin"] = torch.tensor([1, 1, 1, 0, 1, 0, 0, 0, 0], dtype=torch.int32)
    case["cum"][:3] = torch.tensor([-1.5, -2.5, -40.0])
    out, _, _ = run_selection(case)
    check_selection(case, out)
    assert torch.equal(out["cum"][:3], case["cum"][:3]) and out["tok"][:3].tolist() == [PAD] * 3 and out["anc"][:3, SEL_POS].tolist() == [0, 1, 2]
    assert torch.equal(out["len"][:3], case["len"][:3]) and out["fin"][:3].tolist() == [1, 1, 1] and int(out["nfin"][0]) == 3
    assert torch.equal(out["hist"][:3, :SEL_N], case["hist"][:3, :SEL_N])


# ---- engines -----------------------------------------------------------------------------------------------------------------------
# Seeds chosen on the CPU with the oracle's logits (tests/beam_util.py driven by oracle.xformer): no hypothesis of any step holds a
# generated [UNK] (the full-pass yardsticks would inject there, the search does not), hypotheses of 2 .. 21 tokens, 19 of 20 finished,
# and for "small" the restatement alone compares 5 of 5 groups to their end under TOL.
WEIGHTS_SEED, STOP_GAIN = 7, 2.5          # gain of the lm_head's [STOP] row: random weights hardly ever stop
PAYLOAD_SEED = {"small": 2, "hs32": 3, "coati2": 2}          # the injected token payloads of tests 3, 4 and 6
CLIP_SEED = {"small": 2, "hs32": 5}                          # the clip embeddings of test 5


def oracle_params(cfg, seed, stop_gain):
    from oracle import coati_oracle as O
    ocfg = O.OracleConfig(**{k: v for k, v in cfg.items() if k in O.OracleConfig.__dataclass_fields__})
    P = O.init_params(ocfg, seed=seed)
    P["xformer.lm_head.weight"] = P["xformer.lm_head.weight"].clone()
    P["xformer.lm_head.weight"][STOP] *= stop_gain
    return ocfg, P


_ENGINES = {}


def _engine(name, gain=STOP_GAIN):
    key = name
    name = name.split("@")[0]
    if key not in _ENGINES:
        if name == "coati2":
            from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
            torch.manual_seed(3)
            m = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=24, n_tok=48,
                                       enc_to_coati="swiglu_mlp", pad_token=PAD, stop_token=STOP, unk_token=UNK, device=DEV)
            eng = m.engine
            head = [k for k in eng.layout if "lm_head" in k][0]
            eng.view(head)[STOP] *= 2.5
            eng.refresh_shadows()
            _ENGINES[key] = (eng, None, None)
        else:
            from coati_amd.engine import Engine, ModelConfig
            cfg = SMALL if name == "small" else HS32
            ocfg, P = oracle_params(cfg, WEIGHTS_SEED, gain)
            eng = Engine(ModelConfig(**cfg), DEV)
            eng.load_state_dict(P, strict=False)
            _ENGINES[key] = (eng, ocfg, P)
    return _ENGINES[key]


def _payload(G, seed, C=64):
    return torch.randn(G, C, generator=torch.Generator().manual_seed(seed))


def _teacher_forced(eng, tokens, lengths, payload, m=len(PREFIX)):
    """float64 sums of log_softmax over every hypothesis' generated tokens, fed through plain decode_step in a fresh session of the
    same B.  tokens [G, W, T], lengths [G, W], payload [G, C]; the payload is injected where beam_search injects it: in the prefix."""
    G, W, T = tokens.shape
    rows = tokens.reshape(G * W, T).to(DEV)
    inj = payload.to(DEV).repeat_interleave(W, dim=0)
    n = lengths.reshape(G * W).to(DEV)
    total = torch.zeros(G * W, dtype=torch.float64, device=DEV)
    eng.decode_begin(G * W, eng.cfg.n_seq)
    for t in range(T - 1):
        lg = eng.decode_step(rows[:, t].contiguous(), inj if (t < m and int(rows[0, t]) == UNK) else None)
        if t >= m - 1:
            lp = torch.log_softmax(lg.double(), -1).gather(1, rows[:, t + 1:t + 2]).squeeze(1)
            total += torch.where(t + 1 - m < n, lp, torch.zeros_like(lp))
    return total.view(G, W).cpu()


def _check_bookkeeping(tokens, scores, lengths, finished, m=len(PREFIX)):
    """hypotheses of a group pairwise distinct and sorted; finished, lengths and the padding agree with the tokens"""
    G, W, T = tokens.shape
    for g in range(G):
        assert scores[g].tolist() == sorted(scores[g].tolist(), reverse=True)
        assert len({tuple(tokens[g, r].tolist()) for r in range(W)}) == W
        for r in range(W):
            assert tokens[g, r, :m].tolist() == PREFIX
            gen, n = tokens[g, r, m:].tolist(), int(lengths[g, r])
            if bool(finished[g, r]):
                assert gen[n - 1] == STOP and STOP not in gen[:n - 1] and all(t == PAD for t in gen[n:]), (g, r, gen, n)
            else:
                assert n == T - m and STOP not in gen, (g, r, gen, n)


# ---- 3. one beam is greedy decoding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [STOP_GAIN, 1.0], ids=["stopping", "never_stopping"])
@pytest.mark.parametrize("name", ["small", "hs32"])
def test_one_beam_is_greedy_decoding(name, gain):
    """the same logits bit for bit and the same tie rule (value descending, token ascending).  generate_top_k_with_inj_batch overwrites
    the last column of a row that never stopped with [STOP]; beam_search returns such a hypothesis as it stands (its score is that of
    its tokens): the same overwrite is applied here before the exact comparison."""
    eng, _, _ = _engine(name if gain == STOP_GAIN else f"{name}@{gain}", gain)
    payload = _payload(5, PAYLOAD_SEED[name]).to(DEV)
    want = eng.generate_top_k_with_inj_batch(prefix=PREFIX, stop_token=STOP, pad_token=PAD, inv_temp=1.0, k=1, inj_token=UNK,
                                             inj_payload=payload, as_tensor=True).cpu()
    tokens, scores, lengths, finished = (x.cpu() for x in eng.beam_search(PREFIX, STOP, PAD, beams=1, inj_token=UNK, inj_payload=payload))
    assert tokens.shape == (5, 1, want.shape[1])
    got = tokens[:, 0].clone()
    got[~finished[:, 0], -1] = STOP
    assert torch.equal(got, want)
    log(f"one beam vs greedy, {name} gain {gain}: {int(finished.sum())}/5 rows stopped, lengths {lengths[:, 0].tolist()}")
    _check_bookkeeping(tokens, scores, lengths, finished)


def test_refusals_that_need_a_session():
    """a ragged session and a null ancestry table are refused with a code; so is a beam count outside 1 .. 16"""
    from coati_amd import _lib
    eng, _, _ = _engine("small")
    B, T = 4, 24
    tok = torch.full((B,), 20, dtype=torch.long, device=DEV)
    anc = _i32(torch.arange(B).view(B, 1).repeat(1, T))
    eng.decode_begin(B, T)
    eng.decode_step(tok)
    with pytest.raises(RuntimeError, match="null ancestry"):
        _lib.call("coati_engine_decode_step_beams", eng.h, tok.data_ptr(), None, None, None, 0, None)
    assert eng.decode_step_beams(tok, anc).shape == (B, 48) and eng.l.coati_engine_decode_pos(eng.h) == 2
    eng.decode_begin(B, T)
    eng.decode_step_rows(tok, _i32([0] * B))
    with pytest.raises(RuntimeError, match="ragged"):
        eng.decode_step_beams(tok, anc)
    for beams in (0, 17):
        with pytest.raises(ValueError):
            eng.beam_search(PREFIX, STOP, PAD, beams=beams, inj_token=UNK, inj_payload=_payload(2, 0).to(DEV))


# ---- 4. the bookkeeping holds end to end -------------------------------------------------------------------------------------------
_SEARCH = {}


def _search(name, W=4, G=5):
    if (name, W) not in _SEARCH:
        eng, _, _ = _engine(name)
        payload = _payload(G, PAYLOAD_SEED[name])
        trace = []
        side = torch.cuda.Stream(device=DEV)          # what Engine.beam_search does, with the per-step trace of the private loop
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = eng._beam_search(PREFIX, STOP, PAD, W, UNK, payload.to(DEV), None, 0.0, trace=trace)
        torch.cuda.current_stream().wait_stream(side)
        again = eng.beam_search(PREFIX, STOP, PAD, beams=W, inj_token=UNK, inj_payload=payload.to(DEV))
        assert all(torch.equal(a, b) for a, b in zip(out, again))          # the public call returns the same
        _SEARCH[(name, W)] = tuple(x.cpu() for x in out) + (payload, [tuple(x.cpu() for x in step) for step in trace])
    return _SEARCH[(name, W)]


@pytest.mark.parametrize("name", ["small", "hs32", "coati2"])
def test_scores_are_the_teacher_forced_log_likelihoods(name):
    """Every returned hypothesis fed back through plain decode_step: its float64 log_softmax sum equals the returned score within
    1e-4 x length (the logits are the same bits; a single wrong parent anywhere misses this by orders of magnitude)."""
    eng, _, _ = _engine(name)
    tokens, scores, lengths, finished, payload, _ = _search(name)
    _check_bookkeeping(tokens, scores, lengths, finished)
    want = _teacher_forced(eng, tokens, lengths, payload)
    err = (scores.double() - want).abs() / lengths.double()
    log(f"beam search {name}: lengths {int(lengths.min())} .. {int(lengths.max())}, {int(finished.sum())}/{finished.numel()} finished, "
        f"scores {float(scores.min()):.2f} .. {float(scores.max()):.2f}, worst |score - teacher forced| / length {float(err.max()):.2e}")
    assert bool((err <= 1e-4).all()), err
    assert bool(finished.any()) and bool((lengths > 1).any())


def test_length_penalty_only_reorders_and_max_len_cuts():
    eng, _, _ = _engine("small")
    tokens, scores, lengths, finished, payload, _ = _search("small")
    t2, s2, l2, f2 = (x.cpu() for x in eng.beam_search(PREFIX, STOP, PAD, beams=4, inj_token=UNK, inj_payload=payload.to(DEV), length_penalty=1.0))
    key = s2 / l2.clamp(min=1).float()
    for g in range(tokens.shape[0]):
        assert key[g].tolist() == sorted(key[g].tolist(), reverse=True)
        assert sorted(map(tuple, t2[g].tolist())) == sorted(map(tuple, tokens[g].tolist()))
        assert sorted(s2[g].tolist()) == sorted(scores[g].tolist())
    t3, _, l3, f3 = (x.cpu() for x in eng.beam_search(PREFIX, STOP, PAD, beams=4, inj_token=UNK, inj_payload=payload.to(DEV), max_len=6))
    assert t3.shape[2] <= 6 and int(l3.max()) <= 3


# ---- 5. against the full pass ------------------------------------------------------------------------------------------------------
# Measured on code that exists at the parent commit on both sides: max |teacher-forced decode_step sum - Engine.score| over the 20
# hypotheses below (2 .. 21 generated tokens; the step's attention reads its cache, the pass runs the batched kernels; scores of
# -62 .. -4).  The bound is twice it.  |beam score - Engine.score| measured with it: 8.907e-3 (small), 1.002e-2 (hs32).
DECODE_VS_SCORE_GAP = {"small": 8.913e-3, "hs32": 1.003e-2}


@pytest.mark.parametrize("name", ["small", "hs32"])
def test_scores_against_engine_score(name):
    """The hypotheses scored by the full pass (Engine.score: rows from the returned tokens, y_next = -1 on the prefix) against the
    returned scores, within twice the gap between teacher-forced decode_step scoring and Engine.score on these very sequences."""
    from oracle import coati_oracle as O
    eng, ocfg, P = _engine(name)
    G, W = 5, 4
    h_clip = _payload(G, CLIP_SEED[name])
    h_token = O.silu_linear(h_clip, P).detach()
    tokens, scores, lengths, finished = (x.cpu() for x in eng.beam_search(PREFIX, STOP, PAD, beams=W, inj_token=UNK, inj_payload=h_token.to(DEV)))
    m, T = len(PREFIX), tokens.shape[2]
    assert UNK not in tokens[:, :, m:].unique().tolist(), "a generated [UNK]: Engine.score would inject there, the search does not"
    rows = tokens.reshape(G * W, T)
    y = torch.full_like(rows, -1)
    cols = torch.arange(T - 1).view(1, -1)
    keep = (cols >= m - 1) & (cols + 1 - m < lengths.reshape(-1, 1))
    y[:, :-1] = torch.where(keep, rows[:, 1:], y[:, :-1])
    nll = eng.score(rows.to(DEV).contiguous(), y.to(DEV).contiguous(), h_clip=h_clip.repeat_interleave(W, dim=0).to(DEV)).cpu().double()
    forced = _teacher_forced(eng, tokens, lengths, h_token).reshape(-1)
    gap = float((forced + nll).abs().max())
    err = float((scores.reshape(-1).double() + nll).abs().max())
    log(f"beam search {name}: |teacher forced - Engine.score| {gap:.3e} (parent code on both sides), |beam score - Engine.score| {err:.3e}")
    assert err <= 2 * DECODE_VS_SCORE_GAP[name], (gap, err)


# ---- 6. against the restatement on full-prefix logits ------------------------------------------------------------------------------
def restated_search(logits_rows, W, G, steps):
    """beam_util.beam_search per group on logits_rows(g, token lists) -> [n, V]; returns per group (hyps, trace, scales): scales = the
    logit scale (abs max) of every step's rows"""
    out = []
    for g in range(G):
        scales = []

        def fn(gen, g=g, scales=scales):
            lg = logits_rows(g, gen)
            scales.append(float(lg.abs().max()))
            return lg
        hyps, trace = beam_util.beam_search(fn, W, steps, STOP, PAD)
        out.append((hyps, trace, scales))
    return out


def clear_steps(trace, scales):
    """the number of leading steps whose gap between the W-th and the (W+1)-th candidate is at least TOL x the step's logit scale"""
    n = 0
    for (_, gap), scale in zip(trace, scales):
        if gap < TOL * scale:
            break
        n += 1
    return n


def test_search_matches_the_restatement_on_full_prefix_logits():
    """beam_util driven by Engine.decoder_logits (the full pass over every prefix) against Engine.beam_search, per group step by step up
    to the first step at which the restatement's W-th and (W+1)-th candidates are closer than the decode-vs-pass bound; at least three
    quarters of the groups must compare to their end."""
    eng, _, _ = _engine("small")
    G, W, m = 5, 4, len(PREFIX)
    tokens, scores, lengths, finished, payload, trace = _search("small")
    steps = tokens.shape[2] - m

    def logits_rows(g, gen):
        rows = torch.tensor([PREFIX + t for t in gen], dtype=torch.long, device=DEV)
        inj = payload[g:g + 1].to(DEV).expand(rows.shape[0], -1)
        return eng.decoder_logits(rows, inj)[:, -1, :].double().cpu()

    to_end = 0
    for g, (hyps, rtrace, scales) in enumerate(restated_search(logits_rows, W, G, eng.cfg.n_seq - m)):
        n_clear = clear_steps(rtrace, scales)
        for s in range(min(n_clear, len(trace))):
            got = [(int(trace[s][0][g * W + r]) - g * W, int(trace[s][1][g * W + r])) for r in range(W)]
            want = [(p, t) for _, p, t in rtrace[s][0]]
            assert got == want, (g, s, got, want, rtrace[s][1], scales[s])
            assert UNK not in [t for _, t in want], "a generated [UNK]: decoder_logits would inject there, the search does not"
        done = n_clear == len(rtrace)
        if done:
            assert [h[0] for h in hyps] == [tokens[g, r, m:m + len(hyps[0][0])].tolist() for r in range(W)], g
        to_end += done
        log(f"beam search vs restatement, group {g}: {n_clear}/{len(rtrace)} steps clear of the bound")
    assert to_end >= 0.75 * G, to_end


# ---- 7. model level ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_model(golden_dir):
    import coati  # noqa: F401  (the reference's import path)
    from coati.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = np.load(os.path.join(golden_dir, "generation_golden.npz"))
    voc = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=int(g["n_seq"]), smiles_tokens=voc["smiles"] + g["extra_tokens"].tolist(), special_tokens=voc["special"])
    m = e3gnn_smiles_clip_e2e(**SMALL, device=torch.device(DEV))
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "small_model_after3.npz")).items()}
    m.load_state_dict(sd, strict=False)
    return m, tk, g


def test_hclip_to_2d_beam(clip_model):
    from coati_amd.generative import decode_most_likely
    from coati_amd.models.encoding.clip_e2e import injection_prefix
    m, tk, golden = clip_model
    h = torch.randn(3, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    out, toks = m.hclip_to_2d_beam(h, tk, beams=4, return_tokens=True)
    assert len(out) == len(toks) == 3
    prefix = injection_prefix(tk, "[SMILES]", False)
    t, s, n, f = (x.cpu() for x in m.engine.beam_search(prefix, tk.stop_token, tk.pad_token, beams=4, inj_token=tk.unk_token,
                                                       inj_payload=m.special_tokens_from_clip(h)))
    for g in range(3):
        assert len(out[g]) == 4 and all(isinstance(a, str) and isinstance(b, float) for a, b in out[g])
        assert [b for _, b in out[g]] == sorted((b for _, b in out[g]), reverse=True) == s[g].tolist()
        assert toks[g] == [t[g, r, :len(prefix) + int(n[g, r])].tolist() for r in range(4)]
    assert m.hclip_to_2d_beam(h, tk, beams=4) == out == decode_most_likely(m, h, tk, beams=4)
    # point clouds: encode_points, then the same search
    atoms, coords = torch.from_numpy(golden["points.atoms"]).to(DEV), torch.from_numpy(golden["points.coords"]).to(DEV)
    from_points = m.points_to_2d_beam(atoms, coords, tk, beams=3, return_tokens=True)
    assert from_points == m.hclip_to_2d_beam(m.encode_points(atoms, coords), tk, beams=3, return_tokens=True)
    assert len(from_points[0]) == atoms.shape[0] and all(len(x) == 3 for x in from_points[0])
    # one beam: the tokens hclip_to_2d_batch decodes from on the k = 1 path (cut behind [STOP]; a row that never stopped ends in a [STOP]
    # that generate_top_k_with_inj_batch wrote over its last token)
    _, one = m.hclip_to_2d_beam(h, tk, beams=1, return_tokens=True)
    _, greedy = m.hclip_to_2d_batch(h, tk, k=1, return_tokens=True)
    for g in range(3):
        row = greedy[g][:greedy[g].index(tk.stop_token, len(prefix)) + 1]
        if one[g][0][-1] == tk.stop_token:
            assert one[g][0] == row
        else:
            assert one[g][0][:-1] == row[:-1] and len(row) == len(one[g][0])


def test_hcoati_to_2d_beam():
    from coati_amd.generative import decode_most_likely
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from coati_amd.models.simple_coati2.trie_tokenizer import TrieTokenizer
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coati2_vocab.json")) as f:
        v = json.load(f)
    tk = TrieTokenizer(n_seq=v["n_seq"], special_tokens=v["special_tokens"], smiles_tokens=v["smiles_tokens"])
    torch.manual_seed(4)
    m = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=v["n_seq"], enc_to_coati="swiglu_resnet",
                               n_tok=v["ids"]["n_token"], device=DEV)
    h = torch.randn(3, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    out, toks = m.hcoati_to_2d_beam(h, tk, beams=3, return_tokens=True)
    from coati_amd.models.encoding.clip_e2e import injection_prefix
    prefix = injection_prefix(tk, "[SMILES]", False)
    t, s, n, f = (x.cpu() for x in m.engine.beam_search(prefix, tk.stop_token, tk.pad_token, beams=3, inj_token=tk.unk_token,
                                                       inj_payload=m.engine.token_head(h)))
    for g in range(3):
        assert len(out[g]) == 3 and all(isinstance(a, str) and isinstance(b, float) for a, b in out[g])
        assert [b for _, b in out[g]] == s[g].tolist() == sorted(s[g].tolist(), reverse=True)
        assert toks[g] == [t[g, r, :len(prefix) + int(n[g, r])].tolist() for r in range(3)]
    assert decode_most_likely(m, h, tk, beams=3) == out
