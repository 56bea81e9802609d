"""Helpers of tests/test_search4_cpu.py and tests/test_gpu_search4.py: float64 restatements of the four-bit search's first stage on
top of tests/search_util.py (whose oracle, data and tie rule they reuse), the hand-made rows that pin the quantiser, and data that
e2m1 with per-block scales holds exactly."""
import torch

from tests import search_util

NEG_INF = float("-inf")
MIDPOINTS = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -0.0]
MIDPOINT_NIBBLES = [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 8]      # ties go to the even code; the sign is bit 3
STEPS = [1.0, 2.0, 3.0, 4.0, 6.0, -1.0, -2.0, -3.0, -4.0, -6.0, 0.5, 1.5, -0.5, -1.5, 0.0, -0.0]
STEP_NIBBLES = [2, 4, 5, 6, 7, 10, 12, 13, 14, 15, 1, 3, 9, 11, 0, 8]
SPECIAL_ROWS = 11               # quantiser_rows puts this many hand-made rows last (row n - 1 - i is special i)


def query_hat(fp4, queries):
    """f32 [Q, E4]: the dequantised e4m3 queries of Fp4Index.search -- the bf16 query zero-padded to E4, one power-of-two scale each"""
    from coati_amd import fp8_index as F8, search as S
    _, q16 = S.prepare_queries(queries, fp4.metric, fp4.dim, "cpu")
    q16 = torch.nn.functional.pad(q16, (0, fp4.dim_stored - fp4.dim_padded))
    return F8.dequantise(*F8.quantise_rows(q16))


def stage1_scores(fp4, queries, extra=None):
    """([Q, N] float64, q_hat): stage 1's score under the metric, from the DEQUANTISED rows and the dequantised queries
    (search_util.stage1_scores)"""
    q_hat = query_hat(fp4, queries)
    return search_util.stage1_scores(fp4, q_hat, extra), q_hat


def stage1_search(fp4, queries, k, extra=None):
    """the oracle of Fp4Index.search(queries, k, rescore=False): (scores [Q, k] float64, rows [Q, k] int64, the score matrix)"""
    return search_util.stage1_search(fp4, query_hat(fp4, queries), k, extra)


def stage1_ranks(full, rows):
    """[Q, k] int64: the rank (score descending, row ascending among equal scores) that the score matrix `full` gives rows [Q, k]"""
    mine = full.gather(1, rows)
    above = (full[:, None, :] > mine[:, :, None]).sum(dim=2)
    ties_before = ((full[:, None, :] == mine[:, :, None]) & (torch.arange(full.shape[1])[None, None, :] < rows[:, :, None])).sum(dim=2)
    return above + ties_before


def quantiser_rows(n, E, seed):
    """bf16 rows [n, E]: Gaussian ones whose blocks differ in size and, as far as n allows, SPECIAL_ROWS hand-made ones (row n - 1 - i
    is special i; "block 1" only where E >= 64):
      0     a block of zeros (block 0) next to a large one (block 1: 3072 = 6 * 2^9 everywhere);
      1 - 6 for j in (-9, 0, 5): block 0 = 0.5 * 2^j with element 16 = -6 * 2^j (a block maximum of exactly 6 * 2^j), then the same with
            element 16 = 6.03125 * 2^j, the next bf16 value above it (the block exponent steps between the two);
      7     every rounding midpoint in both signs and -0 under a block maximum of 6 (MIDPOINTS at the front of block 0);
      8     STEPS at the front of block 0 and the same values 2^-20 smaller in block 1 (blocks scale independently);
      9     a Gaussian row with -0 in every third place;
      10    a row of -0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, E, generator=g) * torch.exp(3 * torch.randn(n, 1, generator=g))
    x = (x.reshape(n, E // 32, 32) * torch.exp(2 * torch.randn(n, E // 32, 1, generator=g))).reshape(n, E).to(torch.bfloat16)
    special = []
    large = torch.zeros(E)
    large[32:64] = 3072.0
    special.append(large)
    for j in (-9, 0, 5):
        edge = torch.zeros(E)
        edge[:32] = 0.5 * 2.0 ** j
        edge[16] = -6.0 * 2.0 ** j
        special.append(edge)
        above = edge.clone()
        above[16] = 6.03125 * 2.0 ** j                                       # 1.5078125 * 4: the next bf16 value above 6
        special.append(above)
    mid = torch.zeros(E)
    mid[:16] = torch.tensor(MIDPOINTS)
    special.append(mid)
    steps = torch.zeros(E)
    steps[:16] = torch.tensor(STEPS)
    if E >= 64:
        steps[32:48] = torch.tensor(STEPS) * 2.0 ** -20
    special.append(steps)
    negz = torch.randn(E, generator=g)
    negz[::3] = -0.0
    special.append(negz)
    special.append(torch.full((E,), -0.0))
    assert len(special) == SPECIAL_ROWS
    for i, row in enumerate(special[:n]):
        assert torch.equal(row.to(torch.bfloat16).float(), row) or i == 9
        x[n - 1 - i] = row.to(torch.bfloat16)
    return x


def scaled_ints(shape, seed):
    """f32 [N, E]: g * 2^e with g from {0, +-1, +-2, +-3, +-4, +-6} per element and e from -1 .. 2 per (row, block of 32): what e2m1 with
    block scales (and bf16) holds exactly.  Asserted here: against ANY query of integers of magnitude <= 15 the float64 dot and l2
    scores are f32 values -- multiples of 1 / 4 below 2^24 / 4 -- so the kernel's f32 sums are exact whatever their order."""
    N, E = shape
    gen = torch.Generator().manual_seed(seed)
    grid = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, -1.0, -2.0, -3.0, -4.0, -6.0])
    x = grid[torch.randint(0, 11, (N, E), generator=gen)].reshape(N, -1, 32)
    x = (x * 2.0 ** torch.randint(-1, 3, (N, x.shape[1], 1), generator=gen).double()).float().reshape(N, E)
    worst = 2 * 15 * x.double().abs().sum(dim=1) + (x.double() ** 2).sum(dim=1) + 225.0 * E
    assert float(worst.max()) * 4 < 2 ** 24 and bool((x * 4 == (x * 4).round()).all())
    assert torch.equal(worst.float().double(), worst)
    return x


def quat_library(kind, N=4096):
    """one query q = (1024, 256, 64, 16, 4, 1, 0, ...) and rows of six base-4 digits: score = the number the digits spell, exact in
    e2m1, e4m3 and f32.  ascending / descending: the digits of n / of N - 1 - n; constant: (1, 2, 3, 0, 1, 2); blocks: the last digit =
    (n // 100) % 2 under a first digit of 3."""
    n = torch.arange(N)
    x = torch.zeros(N, 32)
    if kind in ("ascending", "descending"):
        v = n if kind == "ascending" else N - 1 - n
        for c in range(6):
            x[:, c] = (v // 4 ** (5 - c)) % 4
    elif kind == "constant":
        x[:, :6] = torch.tensor([1.0, 2.0, 3.0, 0.0, 1.0, 2.0])
    else:
        x[:, 0], x[:, 5] = 3, (n // 100) % 2
    q = torch.zeros(1, 32)
    q[0, :6] = torch.tensor([1024.0, 256.0, 64.0, 16.0, 4.0, 1.0])
    return x, q
