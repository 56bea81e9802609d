"""Property heads, host side (no GPU): include/coati_screen.h parses against coati_hip.h and the library exports what it declares, the
entry refuses bad arguments with a code before any device call, PropertyHead's forward / reference / files / fit, the virtual screen's
control flow on stubs, and the argument checks of EmbeddingIndex.search(bias=) / property_scores / screen."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import screen_util as U  # noqa: E402


# ---- the fifth header -------------------------------------------------------------------------------------------------------
def test_screen_header_parses_into_a_table_of_its_own():
    from coati_amd import _abi, _lib, build
    assert sorted(_lib.SCREEN_PROTOTYPES) == ["coati_head_eval"]
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES):
        assert not set(_lib.SCREEN_PROTOTYPES) & set(other)
    assert "coati_head_eval" not in _lib.exported_symbols()
    assert len(_lib.PROTOTYPES) == 121 and _lib.ABI_VERSION == 5
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib.SCREEN_PROTOTYPES["coati_head_eval"] == (I, [P, L, L, I, P, P, P, P, I, P, P, I, I, P, L, P])
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.SCREEN_HEADER) as f:
        text = f.read()
    again = _abi.parse(text, guard="COATI_SCREEN_H", name="coati_screen.h", base=base)
    assert again.prototypes == _lib.SCREEN_PROTOTYPES and again.version == 5 and not again.experimental
    assert "screen.hip" in build.HIP_UNITS and build.SCREEN_HEADER in build._sources()


def test_library_exports_the_head_entry():
    from coati_amd import _lib
    l = _lib.lib()
    assert l.coati_abi_version() == 5
    for name, (restype, argtypes) in _lib.SCREEN_PROTOTYPES.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_missing_screen_header_is_a_runtime_error_naming_the_path(monkeypatch, tmp_path):
    from coati_amd import _lib, build
    gone = str(tmp_path / "include" / "coati_screen.h")
    monkeypatch.setattr(build, "SCREEN_HEADER", gone)
    try:
        with pytest.raises(RuntimeError, match="coati_screen.h"):
            importlib.reload(_lib)
    finally:
        monkeypatch.undo()
        importlib.reload(_lib)
    assert sorted(_lib.SCREEN_PROTOTYPES) == ["coati_head_eval"]


def test_head_eval_refuses_bad_arguments_with_a_code():
    """decided on the host before any device call: the pointers are host buffers that a refusal never looks at"""
    from coati_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(x=p, ldx=64, N=100, E=64, w0=p, b0=p, wr=p, br=p, D=2, wl=p, bl=p, P=1, F=64, out=p, ldo=1):
        rc = l.coati_head_eval(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, F, out, ldo, None)
        return rc, l.coati_last_error().decode()

    cases = [dict(x=None), dict(w0=None), dict(out=None), dict(b0=None), dict(wl=None), dict(bl=None), dict(wr=None), dict(br=None),
             dict(wr=None, D=1), dict(E=48, ldx=48), dict(E=544, ldx=544), dict(E=0), dict(F=96), dict(F=512), dict(D=-1), dict(D=17),
             dict(P=0), dict(P=9, ldo=9), dict(N=0), dict(N=2 ** 31), dict(ldx=32), dict(ldx=68), dict(P=3, ldo=2),
             dict(x=ctypes.c_void_p(p.value + 2))]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "head_eval" in msg, (kw, rc, msg)


# ---- PropertyHead -------------------------------------------------------------------------------------------------------------
def test_forward_is_the_loop_over_its_own_parameters():
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(0)
    head = PropertyHead(40, features=64, depth=3, num_outputs=2)
    assert len(head.residuals) == 3 and head.first.weight.shape == (64, 40) and head.last.weight.shape == (2, 64)
    x = torch.randn(17, 40)
    h = torch.nn.functional.linear(x, head.first.weight, head.first.bias)
    for res in head.residuals:
        h = h + torch.relu(torch.nn.functional.linear(h, res.weight, res.bias))
    want = torch.nn.functional.linear(h, head.last.weight, head.last.bias)
    got = head(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    xg = x.clone().requires_grad_(True)                       # differentiable with respect to the input
    head(xg).sum().backward()
    assert xg.grad is not None and bool(xg.grad.abs().sum() > 0)
    unit = PropertyHead(40, features=64, depth=3, num_outputs=2, unit_input=True)
    unit.load_state_dict(head.state_dict())
    assert torch.equal(unit(x), head(x / x.norm(dim=1, keepdim=True))) and torch.allclose(unit(3.0 * x), unit(x), atol=1e-5)
    assert head.input_dim_padded == 64 and PropertyHead(256).input_dim_padded == 256


def test_constructor_limits_are_named():
    from coati_amd.models.regression import PropertyHead
    for kw, word in ((dict(input_dim=0), "input_dim"), (dict(input_dim=513), "512"), (dict(features=96), "features"),
                     (dict(features=512), "256"), (dict(depth=-1), "depth"), (dict(depth=17), "16"), (dict(num_outputs=0), "num_outputs"),
                     (dict(num_outputs=9), "8"), (dict(dropout_rate=1.0), "dropout_rate")):
        args = dict(input_dim=64)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            PropertyHead(**args)


def test_reference_has_exactly_the_stated_rounding_points():
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(1)
    head = PropertyHead(40, features=64, depth=2, num_outputs=3)
    x16 = torch.randn(50, 40).to(torch.bfloat16)

    def rb(t):
        return t.detach().float().to(torch.bfloat16).double()

    h = x16.double() @ rb(head.first.weight).T + head.first.bias.detach().double()
    for res in head.residuals:
        h = h + torch.relu(rb(h) @ rb(res.weight).T + res.bias.detach().double())             # the stream itself is not rounded
    want = h @ head.last.weight.detach().double().T + head.last.bias.detach().double()        # nor is the last layer
    got = head.reference(x16)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert torch.equal(head.reference(torch.nn.functional.pad(x16, (0, 24))), want)            # prepared (padded) rows alike
    assert not torch.equal(want, U.unrounded(head, x16))                                      # the roundings are there
    assert head.reference(x16, torch.float32).dtype == torch.float32
    assert float((head.reference(x16, torch.float32).double() - want).abs().max()) < 1e-3 * float(want.abs().max())
    with pytest.raises(ValueError):
        head.reference(x16.float())
    # weights, inputs and every value of the stream exact in bf16: the restatement IS forward, in float64
    exact = U.exact_head(32, 64, 2, 2, seed=5)
    rows = U.exact_rows(200, 32, seed=6)
    fwd = exact.double()(rows.double())
    exact.float()
    assert torch.equal(exact.reference(rows), fwd.detach())


def test_prepare_pads_rounds_and_normalises():
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(100, features=64, depth=1, unit_input=True)
    x = torch.randn(5, 100, dtype=torch.float64)
    x16 = head.prepare(x)
    assert x16.shape == (5, 128) and x16.dtype == torch.bfloat16 and x16.is_contiguous() and bool((x16[:, 100:] == 0).all())
    xf = x.float()
    assert torch.equal(x16[:, :100], (xf / xf.norm(dim=1, keepdim=True).clamp_min(1e-30)).to(torch.bfloat16))
    assert head.prepare(x[0]).shape == (1, 128)
    with pytest.raises(ValueError):
        head.prepare(torch.randn(5, 99))
    with pytest.raises(ValueError):
        head.predict_rows(torch.zeros(3, 100, dtype=torch.bfloat16))                          # not the prepared width
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.predict(x)
    assert head.predict_rows(torch.zeros(0, 128, dtype=torch.bfloat16)).shape == (0, 1)


def test_packed_operands_follow_the_parameters():
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(40, features=64, depth=2, num_outputs=2)
    w0, b0, wr, br, wl, bl = head._operands()
    assert w0.shape == (64, 64) and w0.dtype == torch.bfloat16 and bool((w0[:, 40:] == 0).all())
    assert torch.equal(w0[:, :40], head.first.weight.detach().to(torch.bfloat16))
    assert wr.shape == (2, 64, 64) and wr.dtype == torch.bfloat16 and br.shape == (2, 64) and wl.shape == (2, 64) and wl.dtype == torch.float32
    assert head._operands()[0] is w0                                                           # cached
    with torch.no_grad():
        head.residuals[1].weight.mul_(2.0)
    again = head._operands()
    assert again[0] is not w0 and torch.equal(again[2][1], head.residuals[1].weight.detach().to(torch.bfloat16))
    assert PropertyHead(32, features=64, depth=0)._operands()[2] is None


def test_save_load_round_trip(tmp_path):
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(48, features=128, depth=2, num_outputs=3, unit_input=True, dropout_rate=0.1)
    path = str(tmp_path / "head.pt")
    head.save(path)
    again = PropertyHead.load(path, "cpu")
    assert again.hyper() == head.hyper() and not again.training
    for k, v in head.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k
    x = torch.randn(9, 48)
    assert torch.equal(again(x), head.eval()(x))


def test_fit_recovers_a_linear_property_and_splits_like_the_reference():
    from coati_amd.models.regression import fit_property_head
    rng = np.random.RandomState(3)
    n = 4000
    x = rng.randn(n, 8).astype(np.float32)
    a, c = rng.randn(8).astype(np.float32), 0.7
    y = x @ a + c
    records = [{"emb": x[i], "prop": y[i]} for i in range(n)]
    model, (ys, pred, std) = fit_property_head(records, x_field="emb", y_field="prop", steps=2000, depth=1, features=64, device="cpu")
    np.random.seed(510)
    test_idx = np.random.permutation(n)[:int(0.03 * n)]
    assert std is None and ys.shape == pred.shape == (120,) and np.array_equal(ys, y[test_idx])
    mse, var = float(((pred - ys) ** 2).mean()), float(ys.var())
    print(f"fit: test mse {mse:.4g}, variance of the test targets {var:.4g}")
    assert mse <= 0.1 * var                                    # a constant predictor scores 1.0
    assert model.input_dim == 8 and model.features == 64 and model.depth == 1 and not model.training
    two, (ys2, pred2, _) = fit_property_head(records[:500], x_field="emb", y_field=["prop", "prop"], steps=3, depth=0, features=64, device="cpu")
    assert two.num_outputs == 2 and ys2.shape == pred2.shape == (15, 2)


# ---- the virtual screen on stubs --------------------------------------------------------------------------------------------
class _Maker:
    def __init__(self):
        self.draws = 0

    def rsample(self, shape):
        self.draws += 1
        n = shape[0]
        v = torch.zeros(n, 4)
        v[:, 0] = torch.arange(n).float() + 1000 * self.draws          # a running number, the sample's name
        v[:, 1] = (torch.arange(n) % 4 == 0).float() * 2.0                  # every fourth sample scores 2, the others 0
        return v


class _Head:
    def predict(self, v):
        return v[:, 1:2].clone()


def _stubs(drop=None):
    decode = lambda V: [f"C{int(v[0])}" for v in V]                                       # noqa: E731
    def embed(strings):
        e = torch.zeros(len(strings), 4)
        for i, s in enumerate(strings):
            e[i, 0] = float(s[1:])
            e[i, 1] = 0.5 if drop is not None and drop(int(s[1:])) else 2.0                  # re-embedding may fall under the threshold
        return e
    return decode, embed


def test_virtual_screen_stops_at_n_to_draw():
    from coati_amd.generative import sampled_virtual_screen
    maker = _Maker()
    decode, embed = _stubs()
    hits = sampled_virtual_screen(maker, _Head(), None, None, hit_thresh=1.0, n_to_draw=5, batch_size=8, decode=decode, embed=embed)
    assert [h["smiles"] for h in hits] == ["C1000", "C1004", "C2000", "C2004", "C3000"] and all(h["score"] == 2.0 for h in hits)
    assert maker.draws == 3


def test_virtual_screen_stops_at_max_batches_and_drops_fallen_hits():
    from coati_amd.generative import sampled_virtual_screen
    maker = _Maker()
    decode, embed = _stubs(drop=lambda name: name % 1000 == 0)
    hits = sampled_virtual_screen(maker, _Head(), None, None, hit_thresh=1.0, n_to_draw=50, batch_size=8, max_batches=4, decode=decode,
                                  embed=embed)
    assert maker.draws == 4 and [h["smiles"] for h in hits] == ["C1004", "C2004", "C3004", "C4004"]
    none = sampled_virtual_screen(_Maker(), _Head(), None, None, hit_thresh=5.0, n_to_draw=3, batch_size=8, max_batches=2, decode=decode,
                                  embed=embed)
    assert none == []


def test_generative_and_alias_exports():
    import coati.generative as G
    import coati.models.regression as R
    from coati_amd.generative import coati_screen
    from coati_amd.models.regression import PropertyHead, fit_property_head
    assert G.sampled_virtual_screen is coati_screen.sampled_virtual_screen
    assert R.PropertyHead is PropertyHead and R.fit_property_head is fit_property_head


# ---- EmbeddingIndex: argument checks before any device work -----------------------------------------------------------------
def test_index_argument_checks_come_before_device_work():
    from coati_amd.models.regression import PropertyHead
    from coati_amd.search import EmbeddingIndex
    g = torch.Generator().manual_seed(2)
    index = EmbeddingIndex(40, metric="cosine", device="cpu", keep_f32=True)
    index.add(torch.randn(30, 40, generator=g))
    q = torch.randn(2, 40, generator=g)
    with pytest.raises(ValueError, match="bias"):
        index.search(q, 3, bias=torch.zeros(29))
    with pytest.raises(ValueError, match="bias"):
        index.search(q, 3, bias=torch.zeros(30, dtype=torch.float64))
    with pytest.raises(ValueError, match="rescore"):
        index.search(q, 3, rescore=2, bias=torch.zeros(30))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search(q, 3, bias=torch.zeros(30))                                          # a valid call gets as far as the device
    unit, plain = PropertyHead(40, features=64, depth=1, unit_input=True), PropertyHead(40, features=64, depth=1)
    with pytest.raises(ValueError, match="unit_input"):
        index.property_scores(plain)
    with pytest.raises(ValueError, match="unit_input"):
        EmbeddingIndex(40, metric="dot", device="cpu").property_scores(unit)
    with pytest.raises(ValueError, match="input_dim"):
        index.property_scores(PropertyHead(48, features=64, depth=1, unit_input=True))
    for k in (0, 129):
        with pytest.raises(ValueError, match="k="):
            index.screen(unit, k)
    with pytest.raises(ValueError, match="output"):
        index.screen(unit, 3, output=1)
    with pytest.raises(ValueError, match="unit_input"):
        index.screen(plain, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.screen(unit, 3)
    s, r = EmbeddingIndex(40, metric="cosine", device="cpu").screen(unit, 3)              # an empty index: padding only
    assert s.tolist() == [float("-inf")] * 3 and r.tolist() == [-1] * 3
