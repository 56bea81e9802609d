"""COATI2 training, host side: the feature adds no prototype to include/coati_hip.h; an unbound COATI2 engine -- no gradient or Adam
buffers -- is refused by every step entry before any other check; the new Python keywords, save_coati2 and finetune_coati2 exist;
save_coati2 writes a document the unpickler of load_coati2 reads back; the fixture tests/golden/coati2_train_golden*.npz
(gen_golden_coati2_train.py) is consistent with itself.  Needs no GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ("linear", "swiglu_mlp", "swiglu_resnet")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "coati2_train_golden.npz"))


def test_the_header_still_declares_121_prototypes():
    from coati_amd import _abi
    with open(os.path.join(ROOT, "include", "coati_hip.h")) as f:
        abi = _abi.parse(f.read())
    assert len(abi.prototypes) == 121 and len(abi.experimental) == 5 and abi.version == 5
    for name, n_args in (("coati_engine_forward", 21), ("coati_engine_forward_decoder", 2), ("coati_engine_logits", 4),
                         ("coati_engine_backward", 5), ("coati_engine_optimizer_step", 10), ("coati_engine_workspace_bytes", 6)):
        assert len(abi.prototypes[name][1]) == n_args, name          # unchanged signatures


def test_an_engine_without_training_buffers_is_refused_first():
    """A COATI2 engine that was never bound has no gradient / Adam buffers: every step entry says "inference-only" whatever else is wrong
    with the call (null arguments, no forward), on the host; a COATI1 engine gets the entry's usual first complaint."""
    from coati_amd import _lib
    l = _lib.lib()
    cfg = _lib.CoatiConfig(2, 2, 128, 64, 128, 8, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 0, 1)
    for variant in (0, 1, 2):
        h = ctypes.c_void_p()
        assert l.coati_engine_create_coati2(ctypes.byref(cfg), variant, ctypes.byref(h)) == 0, l.coati_last_error()
        calls = {"engine_forward": lambda: l.coati_engine_forward(h, None, 0, 1, 4, 4, 1, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None),
                 "engine_forward_decoder": lambda: l.coati_engine_forward_decoder(h, None),
                 "engine_logits": lambda: l.coati_engine_logits(h, None, 0, None),
                 "engine_backward": lambda: l.coati_engine_backward(h, None, None, 9, None),
                 "optimizer_step": lambda: l.coati_engine_optimizer_step(h, 1e-3, 0.9, 0.99, 1e-8, 0.1, 10.0, 1, None, None)}
        for entry, call in calls.items():
            assert call() == -1 and b"inference-only" in l.coati_last_error() and entry.encode() in l.coati_last_error(), (entry, l.coati_last_error())
        assert l.coati_engine_workspace_bytes(h, 4, 8, 8, 1, 4) > 0
        l.coati_engine_destroy(h)
    cfg1 = _lib.CoatiConfig(2, 2, 128, 64, 128, 8, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 1, 1)
    h = ctypes.c_void_p()
    assert l.coati_engine_create(ctypes.byref(cfg1), ctypes.byref(h)) == 0
    assert l.coati_engine_backward(h, None, None, 0, None) == -1 and b"inference-only" not in l.coati_last_error()
    l.coati_engine_destroy(h)


def test_new_keywords_and_functions_exist():
    from coati_amd.engine import Engine
    from coati_amd.models.simple_coati2 import io as c2io
    from coati_amd.models.simple_coati2.transformer_only import COATI_Smiles_Inference
    from coati_amd.training import finetune_coati2
    sig = inspect.signature(COATI_Smiles_Inference.__init__)
    assert list(sig.parameters)[-1] == "trainable" and sig.parameters["trainable"].default is False
    assert callable(getattr(COATI_Smiles_Inference, "forward")) and list(inspect.signature(COATI_Smiles_Inference.forward).parameters) == \
        ["self", "raw_tokens", "augmented_tokens", "tokenizer"]
    sig = inspect.signature(c2io.load_coati2)
    assert list(sig.parameters)[-1] == "trainable" and sig.parameters["trainable"].default is False
    assert list(inspect.signature(c2io.save_coati2).parameters) == ["model", "vocab_name", "path", "train_args"]
    p = inspect.signature(finetune_coati2).parameters
    assert list(p)[:8] == ["model", "tokenizer", "smiles", "n_steps", "batch_size", "lr", "do_suffix", "rng"]
    assert p["do_suffix"].default is False and p["rng"].default is None
    f = inspect.signature(Engine.forward).parameters
    assert all(f[k].default is None for k in ("atoms", "coords", "use_point"))
    assert inspect.signature(Engine.train_step).parameters["dh_coati"].default is None
    with pytest.raises(ValueError, match="trainable"):
        finetune_coati2(torch.nn.Linear(2, 2), None, ["C"], 1, 1, 1e-3)


def test_save_coati2_round_trips_through_the_unpickler(tmp_path):
    from coati_amd.models.io.coati import CPU_Unpickler
    from coati_amd.models.simple_coati2.io import save_coati2

    class Stub(torch.nn.Module):          # what save_coati2 reads of a model: model_kwargs and the state_dict
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(3, 2)
            self.register_buffer("mask", torch.tril(torch.ones(4, 4)))
            self.model_kwargs = dict(n_layer_xformer=2, n_hidden_xformer=64, embed_dim=64, n_head=4, n_seq=32, mlp_dropout=0.0,
                                     enc_to_coati="swiglu_resnet", n_direct_clr=64, n_tok=91, biases=True)

    m = Stub()
    path = save_coati2(m, "coati2_12_12", str(tmp_path / "doc.pkl"), train_args={"lr": 1e-4})
    with open(path, "rb") as f:
        doc = CPU_Unpickler(f, encoding="UTF-8").load()
    assert doc["model_kwargs"] == m.model_kwargs and doc["train_args"] == {"lr": 1e-4, "tokenizer_vocab": "coati2_12_12"}
    assert list(doc["model"]) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(doc["model"][k], v) and doc["model"][k].device.type == "cpu", k
    # every key load_coati2 reads of model_kwargs is there
    assert {"n_layer_xformer", "n_hidden_xformer", "embed_dim", "n_head", "n_seq", "mlp_dropout", "enc_to_coati", "n_direct_clr", "n_tok",
            "biases"} <= set(doc["model_kwargs"])


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_gradients_agree_with_their_central_differences(golden, golden_dir, variant):
    """|g| = clip_grad_norm_'s total norm = the norm of the stored per-parameter gradients, and the float64 central difference along g"""
    gv = np.load(os.path.join(golden_dir, f"coati2_train_golden_{variant}.npz"))
    for i in (0, 1):
        n = np.sqrt(sum(float((gv[k].astype(np.float64) ** 2).sum()) for k in gv.files if k.startswith(f"g{i}.")))
        assert abs(n - float(golden[f"{variant}.gradnorm{i}"])) <= 1e-5 * n
        assert abs(n - float(golden[f"{variant}.cd{i}"])) <= 1e-3 * n
    assert sum(k.startswith("g0.") for k in gv.files) == sum(k.startswith("g1.") for k in gv.files) > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_curve_descends_at_the_first_lr_that_does(golden, variant):
    c = golden[f"{variant}.curve"]
    assert c.shape == (20,) and c[-4:].mean() < 0.85 * c[:4].mean()
    assert float(golden[f"{variant}.lr"]) == float(golden["lrs"][0]) == 5e-4       # gen_golden.py's lr already satisfies it
    assert abs(c[0] - float(golden[f"{variant}.ar"])) <= 1e-6 * c[0]
    assert abs(float(golden[f"{variant}.curve_gradnorm"][0]) - float(golden[f"{variant}.gradnorm0"])) <= 1e-6 * float(golden[f"{variant}.gradnorm0"])


def test_fixture_rows(golden, golden_dir):
    lk = np.load(os.path.join(golden_dir, "coati2_likelihood_golden.npz"))
    pad, stop = int(lk["pad_token"]), int(lk["stop_token"])
    for part, B in (("small", 16), ("full", 16)):
        assert np.array_equal(golden[f"{part}.tokens"], lk[f"{part}.tokens"]) and np.array_equal(golden[f"{part}.y_next"], lk[f"{part}.y_next"])
        raw, tok = golden[f"{part}.raw_tokens"], golden[f"{part}.tokens"]
        assert raw.shape[0] == B
        for r, t in zip(raw.tolist(), tok.tolist()):
            n = r.index(stop) + 1
            assert r[0] == 39 and all(x == pad for x in r[n:]) and t[t.index(stop) + 1 - (n - 1):t.index(stop) + 1] == r[1:n]
    assert golden["one.tokens"].shape == (1, 7) and golden["one.raw_tokens"].shape == (1, 5)
    ft, fr, fy = golden["fail.tokens"], golden["fail.raw_tokens"], golden["fail.y_next"]
    assert (ft[1] == pad).all() and (fy[1] == -1).all() and fr[1, 0] == stop and (fr[1, 1:] == pad).all()
    steps = np.load(os.path.join(golden_dir, "coati2_train_golden_steps.npz"))
    assert {k.split(".", 1)[0] for k in steps.files} == {"after1", "after3"}
    for f in os.listdir(golden_dir):
        if f.startswith("coati2_train_golden"):
            assert os.path.getsize(os.path.join(golden_dir, f)) < (1 << 20), f
