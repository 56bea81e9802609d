"""Property heads on the GPU: coati_head_eval (csrc/screen.hip) against PropertyHead.reference -- bit for bit on heads whose sums are
exact, within the summation-order error of f32 on random heads -- its strides and canaries, predict(), and EmbeddingIndex's
property_scores / screen / search(bias=).

Random heads (measured on an MI355X, errors relative to max |reference|): rows within 1e-5: 98.70 % (256, 256, 4, 1), 99.65 % (256, 128, 4, 2),
97.60 % (512, 256, 8, 3), 100 % (32, 64, 1, 1), where the two CPU f32 restatements give 99.15 / 99.15, 99.80 / 99.50, 98.50 / 98.80 and 100 / 100 %;
largest error 9.7e-4 at (512, 256, 8, 3) against the bound 4 x 8.74e-4 taken from the restatements."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import screen_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")

EXACT_SHAPES = [(32, 64, 0, 1), (32, 64, 1, 1), (64, 128, 3, 8), (256, 256, 4, 1), (512, 256, 2, 3)]
EXACT_N = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
RANDOM_SHAPES = [(256, 256, 4, 1), (256, 128, 4, 2), (512, 256, 8, 3), (32, 64, 1, 1)]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. exact heads, bit-equal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_heads_are_bit_equal(shape):
    E, F, D, P = shape
    head = U.exact_head(E, F, D, P, seed=100 + EXACT_SHAPES.index(shape))
    sizes = EXACT_N + ((70001,) if shape == (256, 256, 4, 1) else ())
    rows = U.exact_rows(max(sizes), E, seed=7)
    want = head.reference(rows)
    # every sum is exact in any order: with and without the bf16 rounding of the stream, in float64 and in f32, the same numbers
    assert torch.equal(want, U.unrounded(head, rows)) and torch.equal(want, head.reference(rows, torch.float32).double())
    want = want.float()
    head = head.to(DEV)
    rows_d = rows.to(DEV)
    for n in sizes:
        got = head.predict_rows(rows_d[:n])
        assert got.shape == (n, P) and got.dtype == torch.float32
        bad = (_bits(got.cpu()) != _bits(want[:n])).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, (shape, n, bad[:8].tolist(), got.cpu()[bad[:4]].tolist(), want[bad[:4]].tolist())


# ---- 2. random heads against float64 --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    """per shape: the head, its rows, reference64, and the errors of two CPU f32 restatements (one-piece and 8-chunk K sums)"""
    from coati_amd.models.regression import PropertyHead
    cases, worst = {}, 0.0
    for i, (E, F, D, P) in enumerate(RANDOM_SHAPES):
        torch.manual_seed(20 + i)
        head = PropertyHead(E, features=F, depth=D, num_outputs=P)
        x = torch.randn(2000, E)
        x16 = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        ref = head.reference(x16)
        scale = float(ref.abs().max())
        cpu = []
        for f32 in (head.reference(x16, torch.float32), U.restate_f32_chunked(head, x16)):
            err = (f32.double() - ref).abs().max(dim=1).values / scale
            cpu.append((float((err <= 1e-5).float().mean()), float(err.max())))
            worst = max(worst, float(err.max()))
        cases[(E, F, D, P)] = (head, x16, ref, scale, cpu)
    return cases, worst


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_heads_against_float64(shape, random_cases):
    cases, worst = random_cases
    head, x16, ref, scale, cpu = cases[shape]
    got = head.to(DEV).predict_rows(x16.to(DEV)).cpu()
    head.cpu()
    err = (got.double() - ref).abs().max(dim=1).values / scale
    within, largest = float((err <= 1e-5).float().mean()), float(err.max())
    print(f"head_eval {shape}: rows within 1e-5 of scale {100 * within:.2f} % (CPU f32: {100 * cpu[0][0]:.2f} / {100 * cpu[1][0]:.2f} %), "
          f"largest error {largest:.3g} (CPU f32: {cpu[0][1]:.3g} / {cpu[1][1]:.3g}; bound 4 x {worst:.3g})")
    assert within >= 0.95
    assert largest <= 4 * worst


# ---- 3. strides and canaries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 128, 3, 8), (256, 256, 4, 1)], ids=lambda s: "x".join(map(str, s)))
def test_strides_and_canaries(shape):
    E, F, D, P = shape
    n, extra = 300, 5
    torch.manual_seed(4)
    from coati_amd.models.regression import PropertyHead
    head = PropertyHead(E, features=F, depth=D, num_outputs=P).to(DEV)
    x16 = torch.randn(n, E).to(torch.bfloat16).to(DEV)
    plain = head.predict_rows(x16)
    wide = torch.full((n, E + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, :E] = x16
    view = wide[:, :E]
    assert view.stride(0) == E + 8
    assert torch.equal(_bits(head.predict_rows(view)), _bits(plain))                          # the strided rows are read in place
    canary = torch.full((n + extra, P + 3), float("nan"), dtype=torch.float32, device=DEV).view(torch.int32)
    canary.fill_(0x7FC12345)                                                                  # a NaN pattern
    out = canary.view(torch.float32)
    U.head_eval_raw(head, view, out, n)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:n, :P]), _bits(plain))
    assert bool((canary[:n, P:] == 0x7FC12345).all()) and bool((canary[n:] == 0x7FC12345).all())


# ---- 4. predict -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_input", [False, True])
def test_predict_prepares_the_rows(unit_input):
    from coati_amd.models.regression import PropertyHead
    torch.manual_seed(5)
    head = PropertyHead(100, features=128, depth=2, num_outputs=2, unit_input=unit_input)
    x = torch.randn(333, 100)
    xp = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30) if unit_input else x
    rows = torch.nn.functional.pad(xp.to(torch.bfloat16), (0, 28))
    fwd64 = head.double()(x.double()).detach()
    head.float()
    ref64 = head.reference(rows)
    head.to(DEV)
    got = head.predict(x)                                                                     # f32 vectors on the CPU
    assert got.device.type == "cuda" and got.shape == (333, 2)
    assert torch.equal(_bits(got), _bits(head.predict_rows(rows.to(DEV))))
    bound = 2 * float((ref64 - fwd64).abs().max())
    print(f"predict unit_input={unit_input}: |predict - forward64| {float((got.cpu().double() - fwd64).abs().max()):.3g}, bound {bound:.3g}")
    assert float((got.cpu().double() - fwd64).abs().max()) <= bound
    with torch.no_grad():
        head.last.bias.add_(1.0)
        head.residuals[0].weight.mul_(0.5)
    again = head.predict(x)
    assert not torch.equal(again, got) and float((again.cpu().double() - head.reference(rows.to(DEV)).cpu()).abs().max()) <= bound


# ---- 5. property_scores / screen ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def screened():
    from coati_amd.models.regression import PropertyHead
    from coati_amd.search import EmbeddingIndex
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5000, 256, generator=g)
    x[4950:] = x[100:150]                                                                     # 50 duplicates
    index = EmbeddingIndex(256, metric="cosine", device=DEV)
    index.add(x)
    removed = torch.randperm(5000, generator=g)[:200]
    index.remove(removed)
    torch.manual_seed(7)
    head = PropertyHead(256, features=256, depth=4, num_outputs=2, unit_input=True).to(DEV)
    return index, head, removed


def test_property_scores_and_duplicates(screened):
    index, head, _ = screened
    scores = index.property_scores(head)
    assert scores.shape == (5000, 2) and scores.dtype == torch.float32
    assert torch.equal(_bits(scores[4950:]), _bits(scores[100:150]))                          # equal rows, equal scores
    ref = head.reference(index.vectors).cpu()
    # (the largest error of an f32 restatement in the issue's table is 7.2e-4 of scale; the tight check is test 2's)
    assert float((scores.cpu().double() - ref).abs().max()) <= 4 * 7.2e-4 * float(ref.abs().max())


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_screen_is_the_stable_sort_of_the_live_rows(screened, k, largest):
    index, head, removed = screened
    values = index.property_scores(head)[:, 1].cpu()
    live = torch.ones(5000, dtype=torch.bool)
    live[removed] = False
    rows_live = live.nonzero().flatten()
    order = values[rows_live].sort(descending=largest, stable=True).indices[:k]
    s, r = index.screen(head, k, output=1, largest=largest)
    assert s.shape == (k,) and r.dtype == torch.int64
    assert torch.equal(r.cpu(), rows_live[order])                                             # ties: row ascending
    assert torch.equal(_bits(s.cpu()), _bits(values[rows_live[order]]))                       # the head's own values
    assert not bool(torch.isin(r.cpu(), removed).any())
    # against the float64 restatement: the i-th best value agrees to twice the kernel's error on these rows
    ref = head.reference(index.vectors).cpu()[:, 1]
    eps = float((values.double() - ref).abs().max())
    best = ref[rows_live].sort(descending=largest, stable=True).values[:k]
    assert float((ref[r.cpu()] - best).abs().max()) <= 2 * eps


def test_screen_pads_and_refuses(screened):
    from coati_amd.models.regression import PropertyHead
    from coati_amd.search import EmbeddingIndex
    _, head, _ = screened
    g = torch.Generator().manual_seed(8)
    small = EmbeddingIndex(256, metric="cosine", device=DEV)
    small.add(torch.randn(9, 256, generator=g))
    small.remove([0, 2, 4, 6])
    s, r = small.screen(head, 10)
    assert sorted(r[:5].tolist()) == [1, 3, 5, 7, 8] and r[5:].tolist() == [-1] * 5 and s[5:].tolist() == [-INF] * 5
    assert bool((s[:4] >= s[1:5]).all())
    dot = EmbeddingIndex(256, metric="dot", device=DEV)
    dot.add(torch.randn(9, 256, generator=g))
    with pytest.raises(ValueError, match="unit_input"):
        dot.screen(head, 3)
    l2 = EmbeddingIndex(256, metric="l2", device=DEV)                                       # l2 keeps -|x|^2 in its bias: not part of a screen
    l2.add(torch.randn(40, 256, generator=g))
    plain = PropertyHead(256, features=64, depth=1).to(DEV)
    s, r = l2.screen(plain, 5)
    values = l2.property_scores(plain)[:, 0]
    assert torch.equal(r, values.sort(descending=True, stable=True).indices[:5]) and torch.equal(s, values[r])


# ---- 6. search(bias=) -----------------------------------------------------------------------------------------------------------
def test_search_with_a_bias(screened):
    from coati_amd.search import EmbeddingIndex
    index, head, removed = screened
    g = torch.Generator().manual_seed(9)
    q = torch.randn(7, 256, generator=g)
    s0, r0 = index.search(q, 10)
    s1, r1 = index.search(q, 10, bias=None)
    assert torch.equal(_bits(s0), _bits(s1)) and torch.equal(r0, r1)
    bias = torch.randn(5000, generator=g).mul(0.2).to(DEV)
    bias[r0[0, :3]] = -INF                                                                    # query 0's three nearest are excluded
    s, r = index.search(q, 10, bias=bias)
    other = EmbeddingIndex(256, metric="cosine", device=DEV)
    other.add(torch.zeros(5000, 256))
    other._vec[:5000] = index.vectors
    other._bias[:5000] = index.bias + bias                                                    # the same vector added by hand
    s2, r2 = other.search(q, 10)
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(r, r2)
    assert not bool(torch.isin(r, r0[0, :3]).any()) and not bool(torch.isin(r.cpu(), removed).any())
    # near q and high property, once end to end against torch on the [Q, N] scores
    prop = index.property_scores(head)[:, 0]
    s, r = index.search(q, 10, bias=0.1 * prop)
    q16 = torch.nn.functional.normalize(q, dim=1).to(torch.bfloat16).to(DEV)
    full = q16.double() @ index.vectors.double().T + (index.bias + 0.1 * prop).double()[None]
    want_s, want_r = full.sort(dim=1, descending=True, stable=True)
    assert torch.equal(r, want_r[:, :10])
    assert float((s.double() - want_s[:, :10]).abs().max()) <= 1e-5 * float(want_s[:, :10].abs().max())
