"""Prompt completion and one-sequence generation: the prompt prefill (coati_engine_decode_prefill + kv_cache_fill), the per-row
prompt sampler (coati_topk_sample_prompt) and the model's complete_batch / points_to_2d(_batch) / hclip_to_2d against vectors of the
reference's own methods (tests/golden/generation_golden.npz, gen_golden_generation.py)."""
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
GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
TOL = 7e-3      # bf16 operands, relative to the logit scale (the decode-vs-reference bound of tests/test_gpu_decode.py)
MARGIN = 3e-2   # near-tie rule of test_greedy_generation_matches_reference


def _engine(cfg, seed=1):
    from coati_amd.engine import Engine, ModelConfig
    from oracle import coati_oracle as O
    ocfg = O.OracleConfig(**{k: v for k, v in cfg.items() if k in O.OracleConfig.__dataclass_fields__})
    eng = Engine(ModelConfig(**cfg), DEV)
    eng.load_state_dict(O.init_params(ocfg, seed=seed), strict=False)
    return eng


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _prefill_vs_steps(eng, B, m, inject, label, n_after=10, seed=0):
    """decode_prefill of [B, m] + n_after teacher-forced steps == m + n_after plain steps: logits of position m - 1 and after"""
    c = eng.cfg
    g = torch.Generator().manual_seed(seed)
    T = m + n_after
    toks = torch.randint(12, c.n_tok, (B, T), generator=g)
    inj = None
    if inject:
        toks[:, 1] = c.unk_token
        toks[::3, min(4, m - 1)] = c.unk_token          # a second [UNK] slot in some rows, inside the prompt
        inj = (torch.randn(B, c.n_hidden_xformer, generator=g)).to(DEV)
    toks = toks.to(DEV)
    eng.decode_begin(B, T)
    ref = [eng.decode_step(toks[:, t].contiguous(), inj) for t in range(T)]
    ref = [r.clone() for r in ref[m - 1:]]
    eng.decode_begin(B, T)
    got = [eng.decode_prefill(toks[:, :m], inj).clone()]
    assert eng.l.coati_engine_decode_pos(eng.h) == m
    got += [eng.decode_step(toks[:, t].contiguous(), inj).clone() for t in range(m, T)]
    worst = max(_rel(a, b) for a, b in zip(got, ref))
    log(f"prefill vs steps {label:40s} B={B} m={m}: worst relative logit error {worst:.3e} (tol {TOL:.0e})")
    assert all(torch.isfinite(x).all() for x in got)
    assert worst < TOL, (label, worst)
    return toks, inj


def test_prefill_equals_stepping_small_with_injection():
    eng = _engine(SMALL)
    _prefill_vs_steps(eng, 16, 7, True, "small, injection")
    _prefill_vs_steps(eng, 5, 1, True, "small, m = 1", n_after=3)


def test_prefill_equals_stepping_norm_embed():
    eng = _engine(dict(SMALL, norm_embed=True))
    _prefill_vs_steps(eng, 16, 9, True, "small, norm_embed, injection")


def test_prefill_equals_stepping_grande():
    eng = _engine(GRANDE)
    _prefill_vs_steps(eng, 1024, 40, False, "grande d=256 L=16 V=10322")


def test_prefill_equals_stepping_head_size_32():
    eng = _engine(dict(SMALL, n_hidden_xformer=512, n_embd_common=512, n_head=16, n_seq=64, n_tok=300))
    _prefill_vs_steps(eng, 64, 20, True, "d=512, head size 32, injection")


def test_prefill_then_graph_replay_and_refusals():
    """prefill sets the device position too: captured-graph steps after it equal eager steps bit for bit.  Prefill is refused
    behind a step (the session must be at position 0) and for m > Tmax."""
    eng = _engine(SMALL)
    B, m, T = 8, 6, 14
    toks = torch.randint(12, 48, (B, T), generator=torch.Generator().manual_seed(3)).to(DEV)
    eng.decode_begin(B, T)
    eng.decode_prefill(toks[:, :m])
    eager = [eng.decode_step(toks[:, t].contiguous()).clone() for t in range(m, T)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.decode_begin(B, T)
        eng.decode_graph_build()
        eng.decode_prefill(toks[:, :m])
        for i, t in enumerate(range(m, T)):
            assert torch.equal(eng.decode_step(toks[:, t].contiguous(), graph=True), eager[i]), t
    torch.cuda.current_stream().wait_stream(side)
    eng.decode_begin(B, T)
    eng.decode_step(toks[:, 0].contiguous())
    with pytest.raises(RuntimeError, match="position"):
        eng.decode_prefill(toks[:, :m])
    eng.decode_begin(B, 4)
    with pytest.raises(RuntimeError, match="prompt length"):
        eng.decode_prefill(toks[:, :5])


def test_prefill_refused_on_fp8_generation_falls_back():
    eng = _engine(dict(SMALL, n_hidden_xformer=128, n_embd_common=128, n_head=8, fp8=True))
    eng.decode_begin(2, 8)
    with pytest.raises(RuntimeError, match="fp8"):
        eng.decode_prefill(torch.full((2, 3), 20, dtype=torch.long, device=DEV))
    out = eng.generate_topk_batch([[2, 20, 21], [2, 22]], stop_token=1, k=1)
    assert out[0][:3] == [2, 20, 21] and out[1][:2] == [2, 22] and all(len(r) == 24 for r in out)


# ---- the per-row prompt sampler ------------------------------------------------------------------------------------------
def _sample(logits, k, inv_temp, u, stopped, stop, pad=0):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long, device=DEV)
    _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, V, k, inv_temp, ptr(u), ptr(out), ptr(stopped), stop, pad, stream())
    return out


def _sample_prompt(logits, k, inv_temp, u, prompt, plen, pos, stopped, stop, pad=0):
    from coati_amd import _lib
    from coati_amd.ops import ptr, stream
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long, device=DEV)
    _lib.call("coati_topk_sample_prompt", ptr(logits), logits.stride(0), B, V, k, inv_temp, ptr(u), ptr(prompt), prompt.stride(0), ptr(plen),
              pos, ptr(out), ptr(stopped), stop, pad, stream())
    return out


@pytest.mark.parametrize("V,k", [(300, 5), (10322, 10), (10322, 100), (48, 1)])
def test_prompt_sampler_unforced_rows_are_bit_identical(V, k):
    g = torch.Generator().manual_seed(V + k)
    B = 512
    logits = torch.randn(B, V, generator=g)
    logits[::7, 3] = logits[::7, 5] = 9.0           # ties at the top
    logits = logits.to(DEV)
    u = torch.rand(B, generator=g).to(DEV)
    a = _sample(logits, k, 2.0, u, torch.zeros(B, dtype=torch.int32, device=DEV), stop=-1)
    prompt = torch.randint(0, V, (B, 16), generator=g).to(DEV)
    plen = torch.zeros(B, dtype=torch.int32, device=DEV)
    b = _sample_prompt(logits, k, 2.0, u, prompt, plen, 3, torch.zeros(B, dtype=torch.int32, device=DEV), stop=-1)
    assert torch.equal(a, b)


def test_prompt_sampler_rules():
    """forced rows emit their prompt token; a [STOP] in the prompt flags the row and the row then pads; a sampled stop pads the rest
    of the row; live rows behind their prompt sample"""
    V, B, stop, pad = 64, 6, 1, 0
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(1))
    logits[:, 40] = 50.0                             # arg-max 40 everywhere ...
    logits[4, stop] = 60.0                           # ... except row 4, which draws [STOP]
    logits = logits.to(DEV)
    prompt = torch.tensor([[2, 20, 21, 22], [2, 20, 0, 0], [2, 21, 1, 0], [2, 30, 31, 1], [2, 0, 0, 0], [2, 33, 0, 0]], device=DEV)
    plen = torch.tensor([4, 2, 3, 4, 1, 2], dtype=torch.int32, device=DEV)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    u = torch.zeros(B, device=DEV)
    rows = []
    for pos in range(1, 6):
        rows.append(_sample_prompt(logits, 1, 1.0, u, prompt, plen, pos, st, stop, pad).cpu())
    t = torch.stack(rows, 1)
    assert t[0].tolist() == [20, 21, 22, 40, 40]
    assert t[1].tolist() == [20, 40, 40, 40, 40]
    assert t[2].tolist() == [21, 1, pad, pad, pad]    # [STOP] inside the prompt, then pads
    assert t[3].tolist() == [30, 31, 1, pad, pad]     # [STOP] as the prompt's last token
    assert t[4].tolist() == [1, pad, pad, pad, pad]   # a sampled stop pads the rest
    assert t[5].tolist() == [33, 40, 40, 40, 40]
    assert st.cpu().tolist() == [0, 0, 1, 1, 1, 0]


# ---- parity with the reference ----------------------------------------------------------------------------------------------
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
    behind a row's first mismatch.  Returns (identical, compared, rows fully identical)."""
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


def test_complete_batch_matches_reference(small):
    m, tk, g = small
    prompts = g["prompts"].tolist()
    ref = g["complete.tokens"]
    out = m.xformer.generate_topk_batch([tk.tokenize_text(p, pad=False) for p in prompts], stop_token=tk.stop_token,
                                        pad_token=tk.pad_token, k=1)
    assert len(out) == len(prompts) and all(len(r) == ref.shape[1] for r in out)
    plen = g["complete.plen"]
    for b in range(len(out)):
        assert out[b][: plen[b]] == ref[b][: plen[b]].tolist()       # prompts verbatim
    full = _near_tie_check("complete_batch", out, ref, g["complete.logits"], plen, [ref.shape[1]] * len(out))
    strings = m.complete_batch(prompts, tk, k=1)
    special = m.complete_batch(prompts, tk, k=1, keep_special=True, de_fim=False)
    for b in range(len(out)):
        assert strings[b] == tk.decode(out[b], special=False)
        if full[b]:
            assert strings[b] == g["complete.strings"][b] and special[b] == g["complete.strings_special"][b], b
    stop_row = [b for b in range(len(prompts)) if tk.stop_token in ref[b][: plen[b]].tolist()][0]
    assert out[stop_row] == ref[stop_row].tolist()                   # a prompt with [STOP]: pads behind it


def test_points_to_2d_batch_matches_reference(small):
    m, tk, g = small
    atoms, coords = torch.from_numpy(g["points.atoms"]), torch.from_numpy(g["points.coords"])
    ref = g["points_batch.tokens"]
    strings, toks = m.hclip_to_2d_batch(m.encode_points(atoms.to(DEV), coords.to(DEV)), tk, k=1, keep_special=True, return_tokens=True)
    p = len(g["points_batch.prefix"])
    full = _near_tie_check("points_to_2d_batch", toks, ref, g["points_batch.logits"], [p] * len(toks), [ref.shape[1] - 1] * len(toks))
    assert all(t[-1] == tk.stop_token for t in toks)
    got = m.points_to_2d_batch(atoms.to(DEV), coords.to(DEV), tk, k=1, keep_special=True)
    assert got == strings
    for b in range(len(got)):
        if full[b]:
            assert got[b] == g["points_batch.strings"][b]


def _one_sequence(m, fn):
    """tokens of the one generate_topk_with_inj call fn makes through the model (spy on the engine's bound method)"""
    eng = m.engine
    seen = []
    real = eng.generate_topk_with_inj

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r)
        return r

    eng.generate_topk_with_inj = spy
    try:
        s = fn()
    finally:
        del eng.generate_topk_with_inj
    return seen[0], s


@pytest.mark.parametrize("name", ["points.0", "points.1", "hclip.row", "hclip.vec", "hclip.row_suffix"])
def test_one_sequence_forms_match_reference(small, name):
    """points_to_2d and hclip_to_2d ([1, E] injects the row, [E] its first channel as a scalar over all C; with and without suffix)"""
    m, tk, g = small
    if name.startswith("points"):
        i = int(name[-1])
        atoms, coords = torch.from_numpy(g["points.atoms"][i:i + 1]), torch.from_numpy(g["points.coords"][i:i + 1])
        toks, s = _one_sequence(m, lambda: m.points_to_2d(atoms.to(DEV), coords.to(DEV), tk, k=1))
    else:
        h = torch.from_numpy(g["hclip.in"])
        x = h[1] if name == "hclip.vec" else h[0:1]
        toks, s = _one_sequence(m, lambda: m.hclip_to_2d(x.to(DEV), tk, k=1, do_suffix=name.endswith("suffix")))
    n, p = int(g[f"{name}.len"]), int(g[f"{name}.plen"])
    assert len(toks) <= int(g["n_seq"]) and toks[:p] == g[f"{name}.tokens"][0][:p].tolist()
    full = _near_tie_check(name, [toks + [0] * (int(g["n_seq"]) - len(toks))], g[f"{name}.tokens"], g[f"{name}.logits"], [p], [n])
    if full[0]:
        assert len(toks) == n
        if bool(g[f"{name}.stopped"]):
            assert s == g[f"{name}.string"]


def test_hclip_to_2d_injects_scalar_for_1d_input(small):
    """a 1-D [E] embedding injects the special token's first channel over all C (the reference's h_token[0]): the same tokens as a
    [1, E] embedding whose special token is that constant"""
    m, tk, _ = small
    h = torch.randn(64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    ht = m.special_tokens_from_clip(h.reshape(1, -1))
    prefix = tk.tokenize_text("[CLIP][UNK][SMILES]", pad=False)
    want = m.engine.generate_topk_with_inj(prefix, tk.stop_token, k=1, inj_token=tk.unk_token,
                                           inj_payload=torch.full((64,), float(ht[0, 0]), device=DEV))
    got, _ = _one_sequence(m, lambda: m.hclip_to_2d(h, tk, k=1))
    assert got == want


def test_prefill_and_forced_steps_agree_grande():
    """complete_batch-style prompts of 10..40 tokens at B = 1024, greedy: prefill=True and prefill=False give the same tokens except
    where a near-tie (top-2 margin within the bf16 tolerance, from teacher-forced logits of the prefill=False tokens) flips a draw;
    behind a row's first flip the continuations legitimately differ and are not compared (random weights: flat logits, so over
    ~210 greedy columns per row most rows meet one)"""
    eng = _engine(GRANDE, seed=3)
    g = torch.Generator().manual_seed(4)
    B, n_seq = 1024, GRANDE["n_seq"]
    lens = torch.randint(10, 41, (B,), generator=g).tolist()
    prefix = [[2] + torch.randint(12, GRANDE["n_tok"], (n - 1,), generator=g).tolist() for n in lens]
    a = eng.generate_topk_batch(prefix, stop_token=1, k=1, prefill=True)
    b = eng.generate_topk_batch(prefix, stop_token=1, k=1, prefill=False)
    for r in range(B):
        assert a[r][: lens[r]] == prefix[r] and b[r][: lens[r]] == prefix[r]
    A, Bt = torch.tensor(a), torch.tensor(b)
    diff = (A != Bt)
    rows = torch.nonzero(diff.any(1)).flatten().tolist()
    first = {r: int(torch.nonzero(diff[r]).flatten()[0]) for r in rows}
    if rows:
        # margins where the two first differ: teacher-forced logits of b's tokens
        eng.decode_begin(B, n_seq)
        bt = Bt.to(DEV)
        for t in range(max(first.values())):
            lg = eng.decode_step(bt[:, t].contiguous())
            for r, f in first.items():
                if f == t + 1:
                    top2 = torch.topk(lg[r], 2).values
                    margin = float(top2[0] - top2[1]) / float(lg[r].abs().max())
                    assert margin < MARGIN, (r, f, margin)
    compared = sum((first[r] + 1 if r in first else n_seq) - lens[r] for r in range(B))
    agree = compared - len(rows)
    log(f"grande prefill vs forced steps: {agree}/{compared} generated tokens identical up to each row's first near-tie flip, "
        f"{B - len(rows)}/{B} rows identical")
    assert agree >= 0.9 * compared


def test_generation_leaves_training_untouched():
    """train_step, generation (prefill + prompt sampler), train_step == two train_steps (to the 5e-6 of the step's own float atomics,
    as in the other A/B step tests); generation leaves every flat buffer bit-identical"""
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
                          generator=torch.Generator(device=DEV).manual_seed(0))
    c.generate_topk_with_inj([8, 7, 2], 1, k=1, inj_token=7, inj_payload=torch.randn(64, device=DEV))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(c, k), v), k
    c.train_step(db, up, lr=5e-4)
    Lc = c.losses()
    log(f"train/generate/train vs train/train: {Lc} vs {La}")
    for k in ("ar_loss", "clip_loss", "grad_norm"):
        assert math.isfinite(Lc[k]) and abs(Lc[k] - La[k]) <= 5e-6 * abs(La[k]), (k, Lc, La)
