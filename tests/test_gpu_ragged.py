"""Ragged KV-cached decoding: per-row positions (coati_engine_decode_step_rows, coati_attn_decode_rows), the full prompt prefill on
packed rows (coati_engine_decode_prefill_rows), the ragged sampler (coati_topk_sample_rows), generate_topk_batch(ragged=True) and
Engine.generate_stream (slot refill).  The yardstick everywhere is the existing aligned decode_step; TOL is its own bound."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_util import log  # noqa: E402

DEV = "cuda:0"
SMALL = dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4,
             n_seq=24, n_tok=48)
HS32 = dict(SMALL, n_hidden_xformer=512, n_embd_common=512, n_head=16, n_seq=64, n_tok=300)
GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
TOL = 7e-3      # bf16 operands, relative to the logit scale (the decode bound of tests/test_gpu_generate.py / test_gpu_decode.py)
MARGIN = 3e-2   # near-tie rule of test_complete_batch_matches_reference


def _engine(cfg, seed=1, stop_gain=None):
    from coati_amd.engine import Engine, ModelConfig
    from oracle import coati_oracle as O
    ocfg = O.OracleConfig(**{k: v for k, v in cfg.items() if k in O.OracleConfig.__dataclass_fields__})
    eng = Engine(ModelConfig(**cfg), DEV)
    eng.load_state_dict(O.init_params(ocfg, seed=seed), strict=False)
    if stop_gain is not None:   # random weights hardly ever draw [STOP]: a louder [STOP] row of the lm_head makes rows of many lengths
        name = [k for k in eng.layout if "lm_head" in k][0]
        eng.view(name)[eng.cfg.stop_token] *= stop_gain
        eng.refresh_shadows()
    return eng


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV).contiguous()


def _tokens(c, B, T, g, inject, m=None):
    toks = torch.randint(12, c.n_tok, (B, T), generator=g)
    inj = None
    if inject:
        toks[:, 1] = c.unk_token
        toks[::3, min(4, (m or T) - 1)] = c.unk_token      # a second [UNK] slot in some rows (inside the prompt where there is one)
        inj = torch.randn(B, c.n_hidden_xformer, generator=g).to(DEV)
    return toks, inj


def _aligned(eng, toks, inj):
    """logits [T, B, V] of the aligned session over toks [B, T]"""
    B, T = toks.shape
    eng.decode_begin(B, T)
    return torch.stack([eng.decode_step(toks[:, t].contiguous(), inj).clone() for t in range(T)])


# ---- 1. uniform positions are the old step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,T", [(SMALL, 16, 20), (HS32, 24, 40)], ids=["small", "hs32"])
def test_uniform_positions_are_the_aligned_step_bit_for_bit(cfg, B, T):
    eng = _engine(cfg)
    toks, inj = _tokens(eng.cfg, B, T, torch.Generator().manual_seed(2), True)
    toks = toks.to(DEV)
    ref = _aligned(eng, toks, inj)
    for inj_len in (None, _i32([T] * B)):
        eng.decode_begin(B, T)
        for t in range(T):
            got = eng.decode_step_rows(toks[:, t].contiguous(), _i32([t] * B), inj, inj_len)
            assert torch.equal(got, ref[t]), (t, inj_len is not None)
        assert eng.l.coati_engine_decode_pos(eng.h) == 0       # the session's own position is not used


# ---- 2. ragged prefill + ragged steps against aligned stepping ---------------------------------------------------------------
def _ragged_vs_aligned(eng, B, T, m, lo, inject, label, seed=0):
    c = eng.cfg
    g = torch.Generator().manual_seed(seed)
    toks, inj = _tokens(c, B, T, g, inject, m)
    toks[1, 0] = 0                                           # prompts that contain id 0 ([PAD]) ...
    if lo >= 3:
        toks[2, 2] = 0                                       # ... also inside
    plen = torch.randint(lo, m + 1, (B,), generator=g)
    plen[0], plen[B - 1] = m, lo
    toks = toks.to(DEV)
    ref = _aligned(eng, toks, inj)
    scale = float(ref.abs().max())
    rows = torch.arange(B, device=DEV)
    eng.decode_begin(B, T)
    got = eng.decode_prefill_rows(toks[:, :m], plen, inj)
    pos = plen.to(DEV)
    worst = 0.0
    n_cmp = 0
    for step in range(T - m + 1):
        want = ref[pos - 1, rows]                              # row b against the aligned logits of ITS position
        assert torch.isfinite(got).all(), (label, step)
        err = float((got - want).abs().max()) / scale
        worst = max(worst, err)
        n_cmp += B
        assert err < TOL, (label, step, err)
        if step == T - m:
            break
        tok = toks[rows, pos].contiguous()
        got = eng.decode_step_rows(tok, _i32(pos), inj)
        pos = pos + 1
    log(f"ragged prefill + steps vs aligned {label:34s} B={B} plen {lo}..{m}: {n_cmp} rows compared, worst relative logit error "
        f"{worst:.3e} (tol {TOL:.0e})")


def test_ragged_prefill_and_steps_small_with_injection():
    eng = _engine(SMALL)
    _ragged_vs_aligned(eng, 16, 20, 9, 1, True, "small, injection, plen from 1")
    _ragged_vs_aligned(eng, 16, 20, 9, 3, True, "small, injection, id 0 inside", seed=1)


def test_ragged_prefill_and_steps_norm_embed():
    eng = _engine(dict(SMALL, norm_embed=True))
    _ragged_vs_aligned(eng, 16, 20, 9, 1, True, "small, norm_embed, injection")


def test_ragged_prefill_and_steps_head_size_32():
    eng = _engine(HS32)
    _ragged_vs_aligned(eng, 64, 30, 20, 1, True, "d=512, head size 32, injection")


def test_ragged_prefill_and_steps_grande():
    eng = _engine(GRANDE)
    _ragged_vs_aligned(eng, 1024, 46, 40, 10, False, "grande d=256 L=16 V=10322")


def test_ragged_session_on_a_coati2_engine():
    """the COATI2 decode path (its special ids and parameter table) takes the ragged entries where it takes decode_step"""
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    torch.manual_seed(3)
    m = COATI_Smiles_Inference(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=32, n_tok=80, enc_to_coati="swiglu_mlp",
                               device=DEV)
    eng = m.engine
    B, T = 12, 20
    toks, inj = _tokens(eng.cfg, B, T, torch.Generator().manual_seed(2), True)
    toks = toks.to(DEV)
    ref = _aligned(eng, toks, inj)
    eng.decode_begin(B, T)
    for t in range(T):
        assert torch.equal(eng.decode_step_rows(toks[:, t].contiguous(), _i32([t] * B), inj), ref[t]), t
    _ragged_vs_aligned(eng, 16, 20, 9, 1, True, "COATI2 swiglu_mlp, injection")
    _stream_checks(eng, 4, 3 * 4 + 2, 10, "stream COATI2 k=10")


# ---- 3. idle and refilled slots --------------------------------------------------------------------------------------------
def test_idle_and_refilled_slots():
    """slots 0-2 run from step 0; 3-4 are idle until step 3 and start then; 5-6 run from step 0 and are set back to position 0 at step 5
    with new tokens; 7 stays idle.  Each live row's logits are the aligned reference of the tokens that slot was fed since its
    (re)start; the cache records of idle slots do not change in a step."""
    eng = _engine(SMALL)
    c = eng.cfg
    B, T, steps = 8, 12, 11
    g = torch.Generator().manual_seed(4)
    life = [_tokens(c, B, T, g, True)[0].to(DEV) for _ in range(2)]      # token feeds of a slot's first and second life
    inj = torch.randn(B, c.n_hidden_xformer, generator=g).to(DEV)
    ref = [_aligned(eng, x, inj) for x in life]
    scale = float(ref[0].abs().max())
    start = {0: 0, 1: 0, 2: 0, 3: 3, 4: 3, 5: 0, 6: 0}
    restart = {5: 5, 6: 5}
    eng.decode_begin(B, T)
    L, C = c.n_layer_xformer, c.n_hidden_xformer
    n_cache = L * B * C * T * 2 * 2                                       # bytes of [L][B][nh][Tmax][k | v] bf16, first in the workspace
    cache = lambda: eng._dec_ws[:n_cache].view(L, B, -1).clone()
    eng._dec_ws[:n_cache].random_(0, 255)                                 # whatever idle slots hold, nobody may read or write it
    worst, n_cmp = 0.0, 0
    for s in range(steps):
        pos, which = [], []
        for b in range(B):
            if b in restart and s >= restart[b]:
                pos.append(s - restart[b]); which.append(1)
            elif b in start and s >= start[b]:
                pos.append(s - start[b]); which.append(0)
            else:
                pos.append(-1); which.append(0)
        tok = torch.stack([life[which[b]][b, max(pos[b], 0)] for b in range(B)])
        before = cache()
        got = eng.decode_step_rows(tok, _i32(pos), inj)
        after = cache()
        for b in range(B):
            if pos[b] < 0:
                assert torch.equal(before[:, b], after[:, b]), (s, b)     # an idle slot's cache: not a byte moves
                continue
            assert not torch.equal(before[:, b], after[:, b]), (s, b)
            assert torch.isfinite(got[b]).all(), (s, b)
            err = float((got[b] - ref[which[b]][pos[b], b]).abs().max()) / scale
            worst = max(worst, err)
            n_cmp += 1
            assert err < TOL, (s, b, err)
    log(f"idle / refilled slots: {n_cmp} live rows compared, worst relative logit error {worst:.3e} (tol {TOL:.0e})")


# ---- 4. the ragged sampler ---------------------------------------------------------------------------------------------------
def _sample(logits, k, inv_temp, u, stop):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long, device=DEV)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, V, k, inv_temp, ptr(u), ptr(out), ptr(st), stop, 0, stream())
    return out


def _sample_rows(logits, k, inv_temp, u, ldu, prompt, plen, req, pos, out, tok_next, done, Tmax, stop):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    B, V = logits.shape
    _lib.call("coati_topk_sample_rows", ptr(logits), logits.stride(0), B, V, k, inv_temp, ptr(u), ldu, ptr(prompt),
              prompt.stride(0) if prompt is not None else 0, ptr(plen), ptr(req), ptr(pos), ptr(out), out.stride(0), ptr(tok_next), ptr(done),
              Tmax, stop, stream())


@pytest.mark.parametrize("V,k", [(300, 5), (10322, 10), (10322, 100), (48, 1)])
def test_ragged_sampler_unforced_rows_are_bit_identical(V, k):
    g = torch.Generator().manual_seed(V + k)
    B, W = 512, 16
    logits = torch.randn(B, V, generator=g)
    logits[::7, 3] = logits[::7, 5] = 9.0           # ties at the top
    logits = logits.to(DEV)
    u = torch.rand(B, generator=g).to(DEV)
    want = _sample(logits, k, 2.0, u, stop=-1)
    pos0 = torch.randint(0, W - 2, (B,), generator=g)
    # (a) slot b serves request b, one uniform per slot
    pos, out = _i32(pos0), torch.full((B, W), -5, dtype=torch.long, device=DEV)
    nxt, done = torch.full((B,), -5, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    _sample_rows(logits, k, 2.0, u, 0, None, None, None, pos, out, nxt, done, W, -1)
    assert torch.equal(nxt, want)
    assert torch.equal(out[torch.arange(B), (pos0 + 1).to(DEV)], want) and int((out != -5).sum()) == B
    assert torch.equal(pos.cpu(), (pos0 + 1).to(torch.int32)) and int(done.sum()) == 0
    # (b) slot b serves request req[b]: prompt length, uniform u2[req[b], n] and output row are the request's
    req = torch.randperm(B, generator=g)
    u2 = torch.rand(B, W, generator=g)
    u2[req, pos0 + 1] = u.cpu()
    pos, out = _i32(pos0), torch.full((B, W), -5, dtype=torch.long, device=DEV)
    nxt.fill_(-5)
    plen = torch.zeros(B, dtype=torch.int32, device=DEV)
    prompt = torch.randint(0, V, (B, W), generator=g).to(DEV)
    _sample_rows(logits, k, 2.0, u2.to(DEV), W, prompt, plen, _i32(req), pos, out, nxt, done, W, -1)
    assert torch.equal(nxt, want)
    assert torch.equal(out[req.to(DEV), (pos0 + 1).to(DEV)], want) and int((out != -5).sum()) == B


def test_ragged_sampler_rules():
    """idle slots do nothing; n < plen emits the prompt token (a [STOP] there ends the row); a drawn [STOP] ends the row; a row that
    writes its last column ends; out, the next token vector, the positions and the row lengths against the rule in Python"""
    V, B, W, stop = 64, 8, 6, 1
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(1))
    logits[:, 40] = 50.0                             # arg-max 40 everywhere ...
    logits[4, stop] = 60.0                           # ... except slot 4, which draws [STOP]
    logits = logits.to(DEV)
    prompt = torch.tensor([[2, 20, 21, 22, 0, 0], [2, 20, 0, 0, 0, 0], [2, 21, 1, 23, 0, 0], [2, 30, 31, 1, 0, 0], [2, 0, 0, 0, 0, 0],
                           [2, 33, 0, 0, 0, 0], [2, 34, 35, 36, 37, 38], [2, 0, 0, 0, 0, 0]])
    plen = [4, 2, 4, 4, 1, 2, 6, 1]
    pos = [0, 0, 0, 0, 0, 3, 0, -1]                  # slot 5 starts further on (position 3), slot 7 is idle
    m_out = torch.full((B, W), -5, dtype=torch.long)
    m_nxt, m_done = [-5] * B, [0] * B
    d_pos, d_out = _i32(pos), m_out.clone().to(DEV)
    d_nxt, d_done = torch.full((B,), -5, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    u = torch.zeros(B, device=DEV)
    for _ in range(7):
        _sample_rows(logits, 1, 1.0, u, 0, prompt.to(DEV), _i32(plen), None, d_pos, d_out, d_nxt, d_done, W, stop)
        for b in range(B):                           # the rule
            if pos[b] < 0:
                continue
            n = pos[b] + 1
            tok = int(prompt[b, n]) if n < plen[b] else (stop if b == 4 else 40)
            m_out[b, n] = tok
            m_nxt[b] = tok
            end = tok == stop or n + 1 >= W
            pos[b] = -1 if end else n
            if end:
                m_done[b] = n + 1
        assert d_pos.cpu().tolist() == pos and d_nxt.cpu().tolist() == m_nxt and d_done.cpu().tolist() == m_done
        assert torch.equal(d_out.cpu(), m_out)
    assert pos == [-1] * B
    assert m_out[0].tolist() == [-5, 20, 21, 22, 40, 40] and m_done[0] == 6           # runs into the last column
    assert m_out[2].tolist() == [-5, 21, 1, -5, -5, -5] and m_done[2] == 3            # [STOP] inside the prompt
    assert m_out[4].tolist() == [-5, 1, -5, -5, -5, -5] and m_done[4] == 2            # a drawn [STOP]
    assert m_out[5].tolist() == [-5, -5, -5, -5, 40, 40] and m_done[5] == 6
    assert m_out[7].tolist() == [-5] * 6 and m_done[7] == 0                           # idle: nothing


# ---- 5. generate_topk_batch(ragged=True) against the reference's vectors ----------------------------------------------------------
@pytest.fixture(scope="module")
def small(golden_dir):
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


def _near_tie_check(label, out, ref, ref_logits, start, n):
    """tokens [start[b], n[b]) of every row; a mismatch only where the reference's top-2 margin is within MARGIN, nothing compared
    behind a row's first mismatch (the rule and the 0.9 cap of tests/test_gpu_generate.py)"""
    agree = total = 0
    full = []
    for b in range(len(ref)):
        same = True
        for t in range(int(start[b]), int(n[b])):
            lg = torch.as_tensor(ref_logits[b, t])
            top2 = torch.topk(lg, 2).values
            margin = float(top2[0] - top2[1]) / float(lg.abs().max())
            total += 1
            if int(out[b][t]) == int(ref[b][t]):
                agree += 1
                continue
            assert margin < MARGIN, (label, b, t, margin)
            same = False
            break
        full.append(same and list(out[b][: int(n[b])]) == list(ref[b][: int(n[b])]))
    log(f"{label}: {agree}/{total} tokens identical to the reference, {sum(full)}/{len(full)} rows identical")
    assert agree >= 0.9 * total, label
    return full


def test_ragged_complete_batch_matches_reference(small):
    m, tk, g = small
    prompts = g["prompts"].tolist()
    ref = g["complete.tokens"]
    out = m.xformer.generate_topk_batch([tk.tokenize_text(p, pad=False) for p in prompts], stop_token=tk.stop_token,
                                        pad_token=tk.pad_token, k=1, ragged=True)
    assert len(out) == len(prompts) and all(len(r) == ref.shape[1] for r in out)
    plen = g["complete.plen"]
    for b in range(len(out)):
        assert out[b][: plen[b]] == ref[b][: plen[b]].tolist()       # prompts verbatim
    _near_tie_check("complete_batch, ragged", out, ref, g["complete.logits"], plen, [ref.shape[1]] * len(out))
    stop_row = [b for b in range(len(prompts)) if tk.stop_token in ref[b][: plen[b]].tolist()][0]
    assert out[stop_row] == ref[stop_row].tolist()                   # a prompt with [STOP]: pads behind it


def test_ragged_completion_on_fp8_goes_through_forced_steps():
    eng = _engine(dict(SMALL, n_hidden_xformer=128, n_embd_common=128, n_head=8, fp8=True))
    eng.decode_begin(2, 8)
    with pytest.raises(RuntimeError, match="fp8"):
        eng.decode_prefill_rows(torch.full((2, 3), 20, dtype=torch.long, device=DEV), torch.tensor([3, 2]))
    out = eng.generate_topk_batch([[2, 20, 21], [2, 22], [2, 1, 30]], stop_token=1, k=1, ragged=True)
    assert out[0][:3] == [2, 20, 21] and out[1][:2] == [2, 22] and out[2][:3] == [2, 1, 30] and all(len(r) == 24 for r in out)


# ---- 6. generate_stream by re-scoring -----------------------------------------------------------------------------------------
def _rescore(eng, rows, lens, payload, P, k, label):
    """rows [N, W] teacher-forced through the ALIGNED decode_step (injection at the prefix's [UNK] slot, as _generate feeds it).  At
    every generated position the chosen token's aligned logit must be >= the k-th largest aligned logit - 2 TOL scale (the stream and
    the aligned step are each within TOL of the truth).  The last column of a row that never stopped holds the stop_token the call
    put there, not a draw.  Returns the top-2 margins [N, W] (relative, of the logits that chose column t)."""
    c = eng.cfg
    N, W = rows.shape
    rows_d = rows.to(DEV)
    lens_d = torch.as_tensor(lens).to(DEV)
    eng.decode_begin(N, c.n_seq)
    margins = torch.zeros(N, W)
    n_chk, worst = 0, -1e30
    for t in range(W - 1):
        col = rows_d[:, t].contiguous()
        lg = eng.decode_step(col, payload if (t < P and int(col[0]) == c.unk_token) else None)
        scale = float(lg.abs().max())
        top = torch.topk(lg, max(k, 2)).values
        margins[:, t + 1] = ((top[:, 0] - top[:, 1]) / lg.abs().amax(1)).cpu()
        chosen = lg.gather(1, rows_d[:, t + 1: t + 2]).squeeze(1)
        live = (t + 1 >= P) & (t + 1 < lens_d) & ~((lens_d == c.n_seq) & (t + 1 == c.n_seq - 1))
        slack = (top[:, k - 1] - chosen) / scale
        if bool(live.any()):
            worst = max(worst, float(slack[live].max()))
            n_chk += int(live.sum())
            assert float(slack[live].max()) <= 2 * TOL, (label, t, float(slack[live].max()))
    log(f"{label}: {n_chk} generated tokens re-scored, worst (k-th logit - chosen logit) / scale = {worst:.3e} (bound {2 * TOL:.1e})")
    return margins


def _lens(rows, P, stop):
    """row length = index of the first stop_token behind the prefix + 1 (every row of a stream's result holds one)"""
    out = []
    for r in rows.tolist():
        assert stop in r[P:], "a row without stop_token"
        out.append(P + r[P:].index(stop) + 1)
    return out


def _stream_checks(eng, S, N, k, label, seed=0):
    c = eng.cfg
    prefix = [8, c.unk_token, 2]
    P, stop, pad = len(prefix), c.stop_token, 0
    payload = torch.randn(N, c.n_hidden_xformer, generator=torch.Generator().manual_seed(seed)).to(DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    rows = eng.generate_stream(prefix, stop, pad, 1.0, k, c.unk_token, payload, slots=S, generator=gen(), as_tensor=True).cpu()
    steps = eng.stream_steps
    assert rows.shape[0] == N and rows.shape[1] <= c.n_seq
    lens = _lens(rows, P, stop)
    assert rows.shape[1] == max(lens)                                   # width = the longest row of the call
    for n in range(N):
        r = rows[n].tolist()
        assert r[:P] == prefix                                          # prefix verbatim
        assert all(t == pad for t in r[lens[n]:]) and r[lens[n] - 1] == stop   # pads only behind [STOP]; every row ends in stop_token
    again = eng.generate_stream(prefix, stop, pad, 1.0, k, c.unk_token, payload, slots=S, generator=gen(), as_tensor=True).cpu()
    assert torch.equal(rows, again)                                     # same seed, same result
    lists = eng.generate_stream(prefix, stop, pad, 1.0, k, c.unk_token, payload, slots=S, generator=gen())
    assert lists == rows.tolist()
    margins = _rescore(eng, rows, lens, payload, P, k, label)
    from coati_amd.slots import greedy_steps
    assert steps == greedy_steps([n - 1 for n in lens], min(S, N))      # a row of n tokens occupies its slot for n - 1 steps
    log(f"{label}: N={N} on {S} slots, lengths {min(lens)}..{max(lens)} (mean {sum(lens) / N:.1f}), {steps} steps "
        f"(chunks of {S} through the aligned loop: {sum(max(lens[i:i + S]) - 1 for i in range(0, N, S))})")
    return prefix, payload, rows, lens, margins


def _same_up_to_near_ties(label, got, want, margins, P, lens_want):
    """got / want: token rows; a mismatch only where the aligned top-2 margin (of `want`'s logits) is within MARGIN, nothing compared behind
    a row's first mismatch; at least 0.9 of the compared tokens agree"""
    agree = total = 0
    for b in range(len(want)):
        for t in range(P, lens_want[b]):
            total += 1
            if t < len(got[b]) and int(got[b][t]) == int(want[b][t]):
                agree += 1
                continue
            assert float(margins[b, t]) < MARGIN, (label, b, t, float(margins[b, t]))
            break
    log(f"{label}: {agree}/{total} tokens identical")
    assert agree >= 0.9 * total, label


@pytest.mark.parametrize("k", [1, 10])
def test_generate_stream_small(k):
    eng = _engine(SMALL, seed=5, stop_gain=2.5)
    S, N = 8, 3 * 8 + 5
    prefix, payload, rows, lens, margins = _stream_checks(eng, S, N, k, f"stream small k={k}")
    if k == 1:
        c = eng.cfg
        # request order: row n is what a call with request n alone gives (injection rows all differ)
        for n in (0, 7, 8, 17, N - 1):
            one = eng.generate_stream(prefix, c.stop_token, 0, 1.0, 1, c.unk_token, payload[n:n + 1], as_tensor=True).cpu()
            _same_up_to_near_ties(f"request {n} alone", one.tolist(), rows[n:n + 1].tolist(), margins[n:n + 1], len(prefix), lens[n:n + 1])
        # N <= slots: the aligned batch call's tokens
        want = eng.generate_top_k_with_inj_batch(prefix, c.stop_token, 0, 1.0, 1, c.unk_token, payload[:S], as_tensor=True).cpu()
        got = eng.generate_stream(prefix, c.stop_token, 0, 1.0, 1, c.unk_token, payload[:S], slots=S, as_tensor=True).cpu()
        wl = _lens(want, len(prefix), c.stop_token)
        wm = _rescore(eng, want, wl, payload[:S], len(prefix), 1, "aligned batch call, re-scored")
        _same_up_to_near_ties("stream with N <= slots vs generate_top_k_with_inj_batch", got.tolist(), want.tolist(), wm, len(prefix), wl)


@pytest.mark.parametrize("k", [1, 10])
def test_generate_stream_grande(k):
    eng = _engine(GRANDE, seed=5, stop_gain=3.5)
    _stream_checks(eng, 64, 3 * 64 + 9, k, f"stream grande k={k}")


def test_generate_stream_forced_rows_come_back_in_request_order():
    """every request carries its own forced row (the sampler's prompt rule): the result is exactly those rows, in request order, whatever
    slot and step each ran in; with a look for free slots every 3rd step as well"""
    eng = _engine(SMALL)
    c = eng.cfg
    g = torch.Generator().manual_seed(9)
    N, S, W = 37, 5, 20
    lens = torch.randint(2, W + 1, (N,), generator=g)
    forced = torch.randint(12, c.n_tok, (N, W), generator=g)
    forced[:, 1] = c.unk_token
    forced[torch.arange(N), lens - 1] = c.stop_token
    payload = torch.randn(N, c.n_hidden_xformer, generator=g).to(DEV)
    from coati_amd.slots import greedy_steps
    for poll in (1, 3):
        rows = eng.generate_stream([8], c.stop_token, 0, 1.0, 1, c.unk_token, payload, slots=S, as_tensor=True, poll=poll,
                                   forced=(forced, lens)).cpu()
        assert rows.shape == (N, int(lens.max()))
        for n in range(N):
            assert rows[n, : lens[n]].tolist() == forced[n, : lens[n]].tolist(), n
            assert bool((rows[n, lens[n]:] == 0).all())
        if poll == 1:
            assert eng.stream_steps == greedy_steps((lens - 1).tolist(), S)


# ---- 7. nothing else moves ----------------------------------------------------------------------------------------------------
def test_ragged_generation_leaves_training_untouched():
    """train_step, ragged generation and a stream, train_step == two train_steps (to the 5e-6 of the step's own float atomics, as
    test_generation_leaves_training_untouched); the ragged calls leave every flat buffer bit-identical"""
    from coati_amd.synthetic import make_batch
    b, up = make_batch(16, 20, 6, 48, seed=3, n_special=12, min_len=4, with_rows=True)
    db = {k: (v if k == "rows" else v.to(DEV)) for k, v in b.items()}
    up = up.to(DEV)
    a, c = _engine(SMALL, seed=7), _engine(SMALL, seed=7)
    a.train_step(db, up, lr=5e-4)
    a.train_step(db, up, lr=5e-4)
    La = a.losses()
    c.train_step(db, up, lr=5e-4)
    before = {k: getattr(c, k).clone() for k in ("params", "grads", "adam_m", "adam_v", "shadow")}
    c.generate_topk_batch([[2, 20, 21], [2, 30], [2, 12, 13, 14, 15]], stop_token=1, k=5,
                          generator=torch.Generator(device=DEV).manual_seed(0), ragged=True)
    c.generate_stream([8, 7, 2], 1, 0, 1.0, 5, 7, torch.randn(7, 64, device=DEV), slots=3, generator=torch.Generator(device=DEV).manual_seed(0))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    c.train_step(db, up, lr=5e-4)
    Lc = c.losses()
    log(f"train/ragged generate/train vs train/train: {Lc} vs {La}")
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(Lc[k]) and abs(Lc[k] - La[k]) <= 5e-6 * abs(La[k]), (k, Lc, La)


def test_slots_none_is_the_aligned_path_and_a_number_streams(small):
    m, tk, g = small
    eng = m.engine
    calls = []
    real_batch, real_stream = eng.generate_top_k_with_inj_batch, eng.generate_stream

    def spy_batch(*a, **k):
        calls.append("batch")
        return real_batch(*a, **k)

    def spy_stream(*a, **k):
        calls.append(("stream", k.get("slots")))
        return real_stream(*a, **k)

    eng.generate_top_k_with_inj_batch, eng.generate_stream = spy_batch, spy_stream
    try:
        h = torch.from_numpy(g["hclip.in"]).to(DEV)
        h = torch.cat([h, h + 0.5, h - 0.5])
        a = m.hclip_to_2d_batch(h, tk, k=1)
        assert calls == ["batch"]
        b = m.hclip_to_2d_batch(h, tk, k=1, slots=2)
        assert calls == ["batch", ("stream", 2)]
        assert len(a) == len(b) == h.shape[0]
        from coati_amd.generative.coati_purifications import _decode_repeated
        r0 = _decode_repeated(m, h, tk, 2)
        assert calls[2:] == ["batch"]
        r1 = _decode_repeated(m, h, tk, 2, slots=3)
        assert calls[3:] == [("stream", 3)]
        assert len(r0) == len(r1) == h.shape[0]      # (per-vector results; both routes make their one call whatever it returns)
    finally:
        del eng.generate_top_k_with_inj_batch, eng.generate_stream


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_ragged_refusals():
    from coati_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(**SMALL), DEV)
    tok = torch.full((4,), 20, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="no decode session"):
        eng._dec_B, eng._dec_Tmax = 4, 8
        eng.decode_step_rows(tok, _i32([0] * 4))
    eng = _engine(SMALL)
    prompt = torch.full((4, 5), 20, dtype=torch.long, device=DEV)
    eng.decode_begin(4, 8)
    eng.decode_step(tok)
    with pytest.raises(RuntimeError, match="fresh session"):
        eng.decode_prefill_rows(prompt, torch.tensor([5, 1, 2, 3]))
    eng.decode_begin(4, 8)
    eng.decode_step_rows(tok, _i32([0] * 4))
    with pytest.raises(RuntimeError, match="fresh session"):
        eng.decode_prefill_rows(prompt, torch.tensor([5, 1, 2, 3]))
    eng.decode_begin(4, 8)
    for bad in ([5, 0, 2, 3], [5, 1, 6, 3], [5, 1, 2, -1]):
        with pytest.raises(ValueError, match="prompt lengths"):
            eng.decode_prefill_rows(prompt, torch.tensor(bad))
    eng.decode_begin(4, 4)
    with pytest.raises(ValueError, match="prompt lengths"):
        eng.decode_prefill_rows(prompt, torch.tensor([5, 1, 2, 3]))          # longer than Tmax
    eng.decode_begin(4, 8)
    assert eng.decode_prefill_rows(prompt, torch.tensor([5, 1, 2, 3])).shape == (4, 48)   # and the same call on a fresh session is fine
