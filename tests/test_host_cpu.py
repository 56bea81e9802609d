"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol include/coati_hip.h declares
(no compute calls), the parameter table equals the reference state_dict contract, the synthetic batches and the
clip_ar_xform tail are well-formed, the reference import paths resolve, and the product path refuses to run
without a GPU instead of falling back."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_every_declared_symbol():
    from coati_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "coati_hip.h")).read(), flags=re.S)
    # a count of its own, independent of the header reader the binding is made with (coati_amd/_abi.py): a prototype the reader cannot
    # see is a failure here, not a gap in the binding
    everything = re.findall(r"\b(coati_[a-z0-9_]+)\s*\(", hdr)
    assert len(everything) == len(set(everything)) == len(_lib.PROTOTYPES) and set(everything) == set(_lib.PROTOTYPES)
    if os.environ.get("COATI_AMD_EXPERIMENTAL") != "1":
        hdr = re.sub(r"#ifdef COATI_EXPERIMENTAL.*?#endif", "", hdr, flags=re.S)      # operators of csrc/experimental/: not in the default library
    declared = set(re.findall(r"\b(coati_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    assert l.coati_abi_version() == _lib.ABI_VERSION == 5
    for sym in sorted(declared):
        assert hasattr(l, sym), f"libcoati_hip.so does not export {sym}"
    assert declared == set(_lib.exported_symbols())


def test_bad_arguments_return_codes_not_exceptions():
    from coati_amd import _lib
    l = _lib.lib()
    rc = l.coati_gemm_nt(None, 0, 0, None, 0, 1, 1, 64, None, 0, 0, None, None, None, 0, 0, None)
    assert rc == -1 and b"null" in l.coati_last_error()
    cfg = _lib.CoatiConfig(2, 2, 96, 64, 96, 4, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 1, 1)   # head size 24: unsupported
    h = ctypes.c_void_p()
    assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == -2
    assert b"head size" in l.coati_last_error()


def test_layout_is_the_reference_state_dict_contract(golden_dir):
    from coati_amd import _lib
    from oracle import coati_oracle as O
    l = _lib.lib()
    for kw in (dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48),
               dict(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64, n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48, biases=False),
               dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16, n_seq=250, n_tok=10322)):
        cfg = _lib.CoatiConfig(kw["n_layer_xformer"], kw["n_layer_e3gnn"], kw["n_hidden_xformer"], kw["n_hidden_e3nn"],
                               kw["n_embd_common"], kw["n_head"], kw["n_seq"], kw["n_tok"], 5.0, 0, 1, 7, 0, 1, 1, 1, 1 if kw.get("biases", True) else 0)
        h = ctypes.c_void_p()
        assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
        shapes = O.param_shapes(O.OracleConfig(**kw))
        buf = ctypes.create_string_buffer(256)
        off, rows, cols = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        seen, prev_end = {}, 0
        for i in range(l.coati_engine_n_entries(h)):
            assert l.coati_engine_entry(h, i, buf, 256, ctypes.byref(off), ctypes.byref(rows), ctypes.byref(cols)) == 0
            shape = (rows.value, cols.value) if cols.value > 0 else (rows.value,)
            seen[buf.value.decode()] = shape
            assert off.value % 64 == 0 and off.value >= prev_end
            prev_end = off.value + int(np.prod(shape))
        assert seen == {k: tuple(v) for k, v in shapes.items()}
        assert l.coati_engine_param_elems(h) >= prev_end
        assert l.coati_engine_shadow_elems(h) > l.coati_engine_param_elems(h)
        assert l.coati_engine_workspace_bytes(h, 8, 20, 22, 6, 8) > 0
        l.coati_engine_destroy(h)
    z = np.load(os.path.join(golden_dir, "small_model.npz"))
    assert set(z.files) == set(O.param_shapes(O.OracleConfig(n_layer_e3gnn=2, n_layer_xformer=2, n_hidden_xformer=64,
                                                               n_hidden_e3nn=64, n_embd_common=64, n_head=4, n_seq=24, n_tok=48)))


def test_no_cpu_fallback():
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd import ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine(ModelConfig(), "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm_nt(torch.zeros(4, 64), torch.zeros(4, 64).bfloat16())


def test_periodic_lut_matches_reference_table(golden_dir):
    from coati_amd.periodic import onehot_lut, xy_position
    lut = json.load(open(os.path.join(golden_dir, "constants.json")))["xy_lut"]
    assert all(tuple(lut[z]) == xy_position(z) for z in range(120))
    ix, iy = onehot_lut()
    assert (ix[0], iy[0]) == (27, 17) and (ix[6], iy[6]) == (14, 20) and iy[92] == -1


def test_synthetic_batch_format():
    from coati_amd.synthetic import make_batch, y_next_from_tokens, STOP, PAD, UNK, CLIP
    b, up = make_batch(64, 80, 16, 10322, seed=3)
    assert b["tokens"].shape == (64, 80) and b["raw_tokens"].shape == (64, 78) and b["coords"].dtype == torch.float32
    raw, tok = b["raw_tokens"], b["tokens"]
    assert ((raw == STOP).sum(1) == 1).all()                      # get_stop_token_embs precondition
    good = tok.sum(1) > 0
    assert ((tok[good] == STOP).sum(1) == 1).all()
    assert ((tok == UNK).sum(1) <= 1).all() and (tok[tok[:, 0] == CLIP][:, 1] == UNK).all()
    assert torch.equal(b["y_next"], y_next_from_tokens(tok))
    assert (b["atoms"] >= 0).all() and ((b["atoms"] > 0).sum(1) >= 8).all()
    b2, _ = make_batch(64, 80, 16, 10322, seed=3)
    assert all(torch.equal(b[k], b2[k]) for k in b)


def test_tensorize_tail_matches_reference_xform(golden_dir):
    from coati_amd.models.encoding.clip_e2e import tensorize_batch
    from coati_amd.data.dataset import SyntheticTokenizer
    z = np.load(os.path.join(golden_dir, "xform_tail.npz"))
    tok = torch.from_numpy(z["tokens"])
    raw = torch.from_numpy(z["raw_tokens"])
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 40 - t.shape[1], dtype=t.dtype)], 1)
    out = tensorize_batch({"tokens": pad(tok), "raw_tokens": pad(raw), "atoms": np.array([[6, 6, 8, 0]] * tok.shape[0]),
                           "coords": np.zeros((tok.shape[0], 4, 3))}, SyntheticTokenizer(n_seq=40))
    assert torch.equal(out["tokens"], tok) and torch.equal(out["raw_tokens"], raw)
    assert torch.equal(out["y_next"], torch.from_numpy(z["y_next"]))


def test_reference_import_paths_and_args():
    from coati.training.train_coati import train_autoencoder, do_args, serialize_model  # noqa: F401
    from coati.data.dataset import COATI_dataset
    from coati.models.io.coati import load_e3gnn_smiles_clip_e2e  # noqa: F401
    from coati.models.autograd_funs.autograd_funs import all_gather  # noqa: F401
    from coati.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e, clip_loss  # noqa: F401
    a = do_args([])
    for flag in ("world_size", "nr", "nodes", "gpus", "n_layer_e3gnn", "msg_cutoff_e3nn", "p_clip_emb_smi", "clip_grad",
                 "ngrad_to_save", "resume_document", "tokenizer_vocab", "log_batch_loss", "weight_decay"):
        assert hasattr(a, flag)
    assert (a.lr, a.weight_decay, a.clip_grad, a.n_layer_xformer) == (4e-4, 0.1, 10.0, 16)
    pipe = COATI_dataset(cache_dir=".").get_data_pipe(batch_size=4, distributed_rankmod_total=2, distributed_rankmod_rank=1)
    b = next(iter(pipe))
    assert b["tokens"].shape[0] == 4 and "y_next" in b


def test_stack_batch_matches_reference_golden(golden_dir):
    """the host mirror of coati/data/batch_pipe.py:stack_batch against vectors produced by the reference
    itself (ragged atom counts, a molecule without atoms, flat coordinates)."""
    import numpy as np
    from coati_amd.data.batch_pipe import stack_batch, get_mod_from_str, shard_rows
    g = np.load(os.path.join(golden_dir, "stack_batch.npz"), allow_pickle=False)
    rows = []
    for i, smi in enumerate(g["smiles"]):
        r = {"smiles": str(smi), "source_collection": "x"}
        if f"row{i}_atoms" in g.files:
            r["atoms"] = g[f"row{i}_atoms"]
            r["coords"] = g[f"row{i}_coords"]
        rows.append(r)
    out = stack_batch(rows)
    assert out["atoms"].shape == g["atoms"].shape and out["coords"].shape == g["coords"].shape
    assert np.array_equal(out["atoms"], g["atoms"])
    assert np.array_equal(out["coords"], g["coords"])
    assert [str(x) for x in out["smiles"]] == [str(x) for x in g["smiles"]]
    assert [get_mod_from_str(r["smiles"], 8) for r in rows] == list(g["mods"])
    # the per-rank filter partitions the rows
    parts = [shard_rows(rows, r, 2) for r in range(2)]
    assert sum(len(p) for p in parts) == len(rows)


def test_trie_tokenizer_matches_reference_golden(golden_dir):
    """the C++ trie tokenizer (coati_tokenizer_*) against vectors produced by the reference's
    Trie / TrieTokenizer: splits (incl. the reference's look-ahead quirk on out-of-vocabulary characters), ids, padding,
    KeyError / oversize failures, batch_smiles and decode."""
    import contextlib
    import io
    import json
    from coati_amd.models.encoding.tokenizers import TrieTokenizer, Trie
    g = json.load(open(os.path.join(golden_dir, "tokenizer.json")))
    tk = TrieTokenizer(n_seq=g["n_seq"], smiles_tokens=g["smiles"], special_tokens=g["special"])
    assert tk.n_token == len(g["special"]) + len(g["smiles"]) and tk.stop_token == 1 and tk.unk_token == 7
    for c in g["cases"]:
        assert tk.pre_tokenize(c["text"]) == c["pieces"], c["text"]
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                r = ["ok", tk.tokenize_text(c["text"], pad=True)]
            except KeyError as e:
                r = ["KeyError", str(e)]
            except Exception as e:
                r = ["Exception", str(e.args)]
        assert r == c["result"], (c["text"], r, c["result"])
    with contextlib.redirect_stdout(io.StringIO()):
        bs, bad = tk.batch_smiles(["c1ccccc1", "CxC", "CC(=O)O", "C" * 40, "N(C)C"], skip_failed=True)
    assert bs.tolist() == g["batch_tokens"] and bad == g["batch_bad"]
    okc = [c for c in g["cases"] if c["result"][0] == "ok" and c["text"]][:6]
    dec = [tk.decode(c["result"][1], special=sp) for c in okc for sp in (True, False)]
    assert dec == g["decoded"]
    for c in g["trie_cases"]:
        t = Trie()
        for w in c["words"]:
            t.add(w)
        assert t.split(c["text"]) == c["split"], (c["words"], c["text"])


def test_trie_tokenizer_on_real_vocabulary_slice(golden_dir):
    """The same on a 2 697-token slice of the reference's REAL `may_closedparen` vocabulary (multi-character SMILES fragments,
    overlapping longest matches) and 640 rows: ids of every row, KeyError / oversize rows, batch_smiles on all 640 rows
    (threaded C++ batch encoder) and decode -- vectors written by the reference's TrieTokenizer (gen_golden_tokenizer.py)."""
    import contextlib
    import io
    import json
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    g = json.load(open(os.path.join(golden_dir, "tokenizer_real.json")))
    assert len(g["special"]) + len(g["smiles"]) >= 2000 and len(g["cases"]) >= 500
    assert max(len(t) for t in g["smiles"]) >= 16          # real multi-character fragments, not a toy alphabet
    tk = TrieTokenizer(n_seq=g["n_seq"], smiles_tokens=g["smiles"], special_tokens=g["special"])
    assert tk.n_token == len(g["special"]) + len(g["smiles"])
    assert (tk.pad_token, tk.stop_token, tk.smiles_token, tk.suffix_token, tk.middle_token, tk.unk_token, tk.clip_token) == (0, 1, 2, 5, 6, 7, 8)
    n_ok = 0
    for c in g["cases"]:
        text = "[SMILES]" + c["row"] + "[STOP]"
        if "pieces" in c:
            assert tk.pre_tokenize(text) == c["pieces"], c["row"]
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                r = ["ok", tk.tokenize_text(text, pad=False)]
            except KeyError as e:
                r = ["KeyError", str(e)]
            except Exception as e:
                r = ["Exception", str(e.args)]
        assert r == c["result"], (c["row"], r, c["result"])
        n_ok += r[0] == "ok"
    assert n_ok >= 500
    rows = [c["row"] for c in g["cases"]]
    with contextlib.redirect_stdout(io.StringIO()):
        bs, bad = tk.batch_smiles(rows, skip_failed=True)
    assert bad == g["batch_bad"] and bs.tolist() == g["batch_tokens"]
    okc = [c for c in g["cases"] if c["result"][0] == "ok"][:40]
    assert [tk.decode(c["result"][1], special=sp) for c in okc for sp in (True, False)] == g["decoded"]


def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus N` (the driver's command form) must become N ranks: the script re-executes itself under
    torch.distributed.run.  COATI_BENCH_LAUNCH_CHECK=1 stops each rank after the rendezvous (gloo here, no GPU)."""
    import subprocess
    import sys
    env = dict(os.environ, COATI_BENCH_LAUNCH_CHECK="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert json.loads(line) == {"launch_check": True, "gpus_arg": 2, "world_seen": 2}
    # a launcher that produced another world size than --gpus says is an error, not a silently wrong n_gpus
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=dict(env, WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 4" in (r.stderr + r.stdout)


class _FakeEngine:
    """records the step calls; no device"""

    def __init__(self):
        from coati_amd.engine import Engine
        self.calls = []
        self.layout = {"xformer.emb.tok_emb.weight": (0, (4, 4)), "xformer.transformer.h.0.ln_1.weight": (64, (4,)),
                       "xformer.transformer.h.1.ln_1.weight": (128, (4,)), "xformer.lm_head.weight": (192, (4, 4)),
                       "point_encoder.embedding.weight": (256, (4, 4)), "point_to_clip.0.weight": (320, (4,)),
                       "smiles_to_clip.0.weight": (352, (4,))}
        self.n_params = 384
        import types
        self.cfg = types.SimpleNamespace(use_point_encoder=True, norm_clips=True, token_mlp=True)
        self.grads = torch.arange(384, dtype=torch.float32)
        self.scal = torch.zeros(16)
        self._train_step = Engine.train_step.__get__(self)
        self._eval_step = Engine.eval_step.__get__(self)

    def token_entropy_unit(self):
        return 2.0

    def forward(self, *a, **k):
        self.calls.append(("forward", k.get("train")))
        return torch.ones(3, 4), torch.ones(3, 4), torch.zeros(3, dtype=torch.uint8)

    def forward_decoder(self):
        self.calls.append(("forward_decoder",))

    def contrastive_under_decoder(self, head_fn):
        """host stand-in for Engine.contrastive_under_decoder: the decoder pass is enqueued first, then the contrastive head"""
        self.forward_decoder()
        return head_fn()

    def infonce(self, s, c, sa, ca, bad, row0=0, gscale=1.0):
        self.calls.append(("infonce", row0, gscale, tuple(sa.shape)))
        return torch.ones_like(sa), torch.ones_like(ca)

    def backward(self, dS, dC, stage=0):
        self.calls.append(("backward", stage))

    def optimizer_step(self, lr, **kw):
        self.calls.append(("optimizer_step", lr, kw))


def test_optimizer_arguments_reach_the_optimizer():
    """--weight_decay / --clip_grad (train_coati.py:145-151, 276) must arrive at Engine.optimizer_step on both the
    single-GPU and the data-parallel step; the evaluation step runs forward + InfoNCE only."""
    import torch.distributed as dist
    from coati_amd import distributed as D
    batch = {k: torch.zeros(3, 5, dtype=torch.long) for k in ("raw_tokens", "tokens", "atoms", "y_next")}
    batch["coords"] = torch.zeros(3, 5, 3)
    up = torch.ones(3, dtype=torch.bool)
    e = _FakeEngine()
    e._train_step(batch, up, 1e-3, weight_decay=0.03, max_norm=2.0)
    assert e.calls[-1] == ("optimizer_step", 1e-3, {"weight_decay": 0.03, "max_norm": 2.0})
    e.calls.clear()
    e._eval_step(batch, up)
    assert [c[0] for c in e.calls] == ["forward", "infonce"] and e.calls[0] == ("forward", False)
    store = dist.HashStore()
    dist.init_process_group("gloo", rank=0, world_size=1, store=store)
    try:
        e.calls.clear()
        D.distributed_train_step(e, batch, up, 2e-3, weight_decay=0.07, max_norm=3.0)
        names = [c[0] for c in e.calls]
        # decoder stage | ONE encoder stage (the pass's weight gradients are one grouped launch) | point-encoder stage
        # (the contrastive head is enqueued BEHIND the decoder pass's launches: it runs on a side stream underneath them)
        assert names == ["forward", "forward_decoder", "infonce", "backward", "backward", "backward", "optimizer_step"]
        assert [c[1] for c in e.calls if c[0] == "backward"] == [1, 2, 3]
        assert e.calls[-1] == ("optimizer_step", 2e-3, {"weight_decay": 0.07, "max_norm": 3.0})
        # the round-1 schedule (encoder stage in two halves) stays available behind COATI_DP_SPLIT=1
        D._SPLIT_ENCODER_STAGE = True
        try:
            e.calls.clear()
            D.distributed_train_step(e, batch, up, 2e-3)
            assert [c[1] for c in e.calls if c[0] == "backward"] == [1, 4, 5, 3]
        finally:
            D._SPLIT_ENCODER_STAGE = False
        # the five buckets tile the flat gradient buffer exactly once
        bk = sorted(D.grad_buckets(e).values())
        assert bk[0][0] == 0 and bk[-1][1] == e.n_params and all(a[1] == b[0] for a, b in zip(bk, bk[1:]))
        e.calls.clear()
        D.distributed_eval_step(e, batch, up)
        assert [c[0] for c in e.calls] == ["forward", "infonce"]
        assert D.all_agree(True, "cpu") and not D.all_agree(False, "cpu")
    finally:
        dist.destroy_process_group()


def test_measured_dp_schedule_is_per_engine_and_decided_once(monkeypatch):
    """The run-time choice between {one encoder stage, two halves, two halves + bf16 wire} (coati_amd.distributed._Schedule): 3 warm-up
    steps, 3 timed steps of each candidate (device events), MAX over ranks, then the winner for good (the bf16 wire only when it is
    more than WIRE_MARGIN ahead of the best fp32 candidate) -- with the backend check and the device
    events replaced by host stand-ins so that the counters, the vote and the decision run on CPU.  The state belongs to the
    engine: a second engine starts its own measurement, an evaluation step in between does not advance it."""
    import torch.distributed as dist
    from coati_amd import distributed as D
    batch = {k: torch.zeros(3, 5, dtype=torch.long) for k in ("raw_tokens", "tokens", "atoms", "y_next")}
    batch["coords"] = torch.zeros(3, 5, 3)
    up = torch.ones(3, dtype=torch.bool)
    clock = {"t": 0.0, "cost": {False: 5.0, True: 3.0}}     # ms per step of the two forms: the split form is faster here

    class FakeEvent:
        def __init__(self, enable_timing=False):
            self.t = None

        def record(self):
            self.t = clock["t"]

        def elapsed_time(self, other):
            return other.t - self.t

    monkeypatch.setattr(D, "_measurable", lambda: True)
    monkeypatch.setattr(D, "_SPLIT_ENV", None)
    monkeypatch.setattr(D, "_WIRE_ENV", None)
    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(D, "control_group", lambda: None)
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        def run(e):
            e.calls.clear()
            real_backward = e.backward

            def backward(dS, dC, stage=0):
                if stage in (2, 4):      # the encoder stage is where the two forms differ
                    clock["t"] += clock["cost"][stage == 4]
                return real_backward(dS, dC, stage)
            e.backward = backward
            D.distributed_train_step(e, batch, up, 1e-3)
            e.backward = real_backward
            return [c[1] for c in e.calls if c[0] == "backward"]

        e1, e2 = _FakeEngine(), _FakeEngine()
        seq = [run(e1) for _ in range(3)]
        assert seq == [[1, 2, 3]] * 3                              # warm-up: one piece, untimed
        D.distributed_eval_step(e1, batch, up)                      # an evaluation step does not advance the measurement
        assert [run(e1) for _ in range(3)] == [[1, 2, 3]] * 3      # form 0 timed
        assert run(e2) == [1, 2, 3] and e2._dp_schedule.step == 1   # another engine: its own counters
        assert [run(e1) for _ in range(3)] == [[1, 4, 5, 3]] * 3   # form 1 timed
        assert not e1._dp_schedule.decided
        assert [run(e1) for _ in range(3)] == [[1, 4, 5, 3]] * 3   # form 2 (two halves + bf16 wire) timed
        # 3 ms < 5 ms: two halves; the bf16 wire is no faster here (the stand-in has no wire), so the fp32 wire stays
        assert e1._dp_schedule.decided and e1._dp_schedule.split and e1._dp_schedule.wire == "fp32"
        assert run(e1) == [1, 4, 5, 3] and run(e1) == [1, 4, 5, 3]
        assert not e2._dp_schedule.decided
        clock["cost"] = {False: 2.0, True: 3.0}                    # on e2 the one-piece form wins
        for _ in range(11):
            run(e2)
        assert e2._dp_schedule.decided and not e2._dp_schedule.split and run(e2) == [1, 2, 3]
    finally:
        dist.destroy_process_group()


def test_dp_schedule_candidates_and_pick():
    """what the vote runs over, and the rule it decides by (every rank applies it to the same MAX-reduced numbers)"""
    from coati_amd import distributed as D
    three = [(False, "fp32"), (True, "fp32"), (True, "bf16")]
    assert D.schedule_candidates(None, None) == three
    assert D.schedule_candidates("0", None) == [(False, "fp32"), (False, "bf16")]
    assert D.schedule_candidates(None, "fp32") == [(False, "fp32"), (True, "fp32")]
    assert D.schedule_candidates("1", "bf16") == [(True, "bf16")]
    assert D.schedule_candidates(None, "bf16") == [(True, "bf16")]
    assert D.schedule_pick(three, [10.0, 9.0, 8.9]) == 1            # bf16 1 % ahead: not worth a rounding per element
    assert D.schedule_pick(three, [10.0, 9.0, 8.5]) == 2            # 5.6 % ahead
    assert D.schedule_pick(three, [8.0, 9.0, 8.5]) == 0
    assert D.schedule_pick(three, [9.0, 9.0, 9.0]) == 0             # ties go to the first (simplest) candidate
    assert D.schedule_pick([(True, "bf16")], [1.0]) == 0


def test_grad_buckets_tile_the_buffer_for_every_flag_layout():
    """grad_buckets on layouts as build_layout (csrc/engine.cpp) produces them for the constructor flags: torch_emb renames the
    point encoder's first entry (`emb.weight`, round-5 advisor: a hard-coded `embedding.weight` raised KeyError under data
    parallelism), use_point_encoder=False moves the point encoder behind the trainable range"""
    from coati_amd import distributed as D
    import types

    def eng(pe_key, pe_first=True):
        lay = {"xformer.emb.tok_emb.weight": (0, (4, 4)), "xformer.transformer.h.0.ln_1.weight": (64, (4,)),
               "xformer.transformer.h.1.ln_1.weight": (128, (4,))}
        if pe_first:
            lay.update({pe_key: (192, (4, 4)), "point_encoder.node_dec.0.weight": (224, (4, 4)), "xformer.lm_head.weight": (256, (4, 4)),
                        "point_to_clip.0.weight": (320, (4,)), "smiles_to_clip.0.weight": (352, (4,))})
        else:
            lay.update({"xformer.lm_head.weight": (192, (4, 4)), "smiles_to_clip.0.weight": (256, (4,)), pe_key: (320, (4, 4)),
                        "point_encoder.node_dec.0.weight": (352, (4, 4))})
        return types.SimpleNamespace(layout=lay, n_params=384)
    for key in ("point_encoder.embedding.weight", "point_encoder.emb.weight"):
        for first in (True, False):
            bk = D.grad_buckets(eng(key, first))
            r = sorted(bk.values())
            assert r[0][0] == 0 and r[-1][1] == 384 and all(a[1] == b[0] for a, b in zip(r, r[1:])), (key, first, bk)
            assert bk["gnn"][0] == (192 if first else 320)
            assert set(D.wire_bytes_per_rank(eng(key, first), "bf16")) == set(bk)


def test_trainer_passes_args_to_the_step():
    """the trainer hands args.weight_decay / args.clip_grad to every training step and evaluates forward-only"""
    import inspect
    from coati_amd.training import train_coati as T
    src = inspect.getsource(T.train_autoencoder)
    assert "weight_decay=float(args.weight_decay)" in src and "max_norm=float(args.clip_grad)" in src
    assert "eval_step" in src and "distributed_eval_step" in src and "**opt_kw" in src


def test_comm_entries_reject_bad_arguments_without_a_gpu():
    """coati_comm_*: argument checks come before RCCL is touched (no GPU, possibly no librccl, here)"""
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_comm_unique_id(None, 128) == -1
    assert l.coati_comm_unique_id(ctypes.create_string_buffer(16), 16) == -1 and b"128" in l.coati_last_error()
    assert l.coati_comm_init(None, 0, 1, None) == -1
    uid = ctypes.create_string_buffer(128)
    assert l.coati_comm_init(uid, 2, 2, ctypes.byref(ctypes.c_void_p())) == -1 and b"rank 2 of 2" in l.coati_last_error()
    assert l.coati_allgather_rows(None, None, None, 1, 1, 0, None) == -1
    assert l.coati_comm_rank(None) == -1 and l.coati_comm_world(None) == -1 and l.coati_comm_destroy(None) == 0


def test_attention_score_efficiency_of_the_bench_workload():
    """bench.py's `attention.useful_over_computed`: on 16-row causal granularity (csrc/attention16.hip) the headline workload's two passes
    evaluate < 1.67 x the score elements of the causal triangle (round 5, 32-row blocks: 2.4 x) -- a regression of the kernel's
    granularity, or of the metric, is red here"""
    from coati_amd.synthetic import attention_score_efficiency, make_batch, packed_lengths
    b, _ = make_batch(1024, 80, 16, 10322, seed=1234, with_rows=True)
    l1, l2 = packed_lengths(b["raw_tokens"], b["tokens"], b["y_next"])
    e16, e32 = attention_score_efficiency(torch.cat([l1, l2]), 16), attention_score_efficiency(torch.cat([l1, l2]), 32)
    assert e16 >= 0.6 and 0.38 <= e32 <= 0.46 and e16 > 1.4 * e32, (e16, e32)
    assert attention_score_efficiency(torch.tensor([16, 32]), 16) == (136 + 528) / (256.0 * 4)
    assert attention_score_efficiency(torch.tensor([0, 17]), 16) == 153 / (256.0 * 3)


def test_committed_step_traffic_does_not_regress():
    """`_step.hbm_GB_per_step` of the newest committed PMC summary (profiles/rNN_pmc_summary.json: rocprofv3 FETCH_SIZE / WRITE_SIZE passes over
    the bench command, tools/profile_round.sh): the step's HBM traffic must not creep up from round to round unnoticed.  The bound is
    the round-5 value (88.06 GB) + 2 %; the kernels the bench line's `roofline.traffic` names must be in the summary."""
    import glob
    import json
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r*_pmc_summary.json")))
    assert files, "no PMC summary committed"
    d = json.load(open(files[-1]))
    assert "_step" in d and "dgrad_lnbwd" in d and "xf_wgrad" in d, (files[-1], list(d))
    step = d["_step"]
    assert abs(step["hbm_read_GB_per_step"] + step["hbm_write_GB_per_step"] - step["hbm_GB_per_step"]) < 0.05
    assert step["hbm_GB_per_step"] <= 88.06 * 1.02, (files[-1], step["hbm_GB_per_step"])


def test_a_probe_build_does_not_pass_for_the_product(monkeypatch):
    """coati_amd/build.py: the library carries the compiler flags it was built with (libcoati_hip.so.flags); with other flags in the
    environment's COATI_AMD_CXXFLAGS -- a probe build's -D switches -- or without the stamp, an un-forced build() rebuilds.  (Round 6: a
    -DR16_TURNS=3 library survived `python coati_amd/build.py` because only source times were compared, and gave NaN at 9-10 waves.)"""
    from coati_amd import build as B
    B.build(verbose=False)            # (builds only if the library is missing or stale)
    assert os.path.exists(B.LIB) and os.path.exists(B._stamp_path())
    assert open(B._stamp_path()).read() == " ".join(B.FLAGS)
    assert not B.needs_build()
    monkeypatch.setattr(B, "FLAGS", B.FLAGS + ["-DR16_TURNS=3"])
    assert B.needs_build()


def test_environment_table_lists_exactly_what_the_sources_read():
    """INTEGRATION.md "Environment switches" against the sources: every COATI_* name that is a string literal argument of getenv( in
    coati_amd/csrc/ or of os.environ.get( / os.environ[ in the package has a row, and no row names a variable nothing reads.  The default
    library (csrc/ without experimental/) reads three: the two A/B switches whose other path a test runs as its reference, and the RCCL
    path; a new switch there has to be argued for here."""
    import glob
    pkg = os.path.join(ROOT, "coati_amd")
    cxx = {}
    for ext in ("hip", "cpp", "h"):
        for path in glob.glob(os.path.join(pkg, "csrc", "**", "*." + ext), recursive=True):
            cxx[os.path.relpath(path, os.path.join(pkg, "csrc"))] = set(re.findall(r'\bgetenv\(\s*"(COATI_[A-Z0-9_]+)"', open(path).read()))
    py = set()
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        py |= set(re.findall(r'\b_?os\.environ(?:\.get\(|\[)\s*["\'](COATI_[A-Z0-9_]+)["\']', open(path).read()))
    default_build = set().union(*(names for rel, names in cxx.items() if not rel.startswith("experimental" + os.sep)))
    assert default_build == {"COATI_NO_TAIL", "COATI_NO_LNBWD_FUSE", "COATI_RCCL_LIB"}, sorted(default_build)
    read = set().union(py, *cxx.values())
    section = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    rows = [line.split("|")[1] for line in section.splitlines() if line.startswith("|")]
    table = set(re.findall(r"COATI_[A-Z0-9_]+", " ".join(rows)))
    assert table and read == table, (sorted(read - table), sorted(table - read))
