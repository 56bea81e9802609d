"""The radius search (coati_radius_count / coati_radius_fill through coati_amd.radius) against the exact search's kernel on the same
library: per library (4 M rows x 256 and 1 M rows x 512, bf16, Gaussian, metric "dot"), Q in {1, 64, 1024} and thresholds that hit about
0, about 100 and about 10 000 rows per query (the score of a Gaussian row is N(0, |q|^2): the threshold is |q| times the normal quantile
of 1 - hits / N; the hits counted are reported), in one process and alternated round by round,
  (a) coati_radius_count on prepared buffers                        the count pass alone;
  (b) count, prefix sum, .item(), allocation, coati_radius_fill     radius.Operands.search: what radius_search costs behind the queries'
      preparation, its one synchronisation included;
  (c) coati_search_topk k = 1 and (d) k = 128 on prepared buffers   the yardstick: the exact search's kernel + merge.
Then, on a 1 M x 256 "cosine" library, the near-duplicate self-join at a threshold nothing but a row itself reaches, with the triangle
(row_hi[i] = i: near_duplicates) and as the full square (no row bound), and per threshold the share of the fill pass's workgroups that
leave at once because their tile has no hit in their slice.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds.
    python tools/radius_bench.py [--reps 5] [--inner 10] [--small] [--out profiles/radius_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib, radius  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("radius_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256), (1 << 20, 512)]
QS, HITS = (1, 64, 1024), (0, 100, 10000)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def early_share(counts, Q, S, np_queries=64):
    """the share of the fill pass's (tile, slice) workgroups whose tile has no hit in the slice"""
    tiles = -(-Q // np_queries)
    padded = torch.zeros(tiles * np_queries, S, dtype=counts.dtype, device=counts.device)
    padded[:Q] = counts
    return float((padded.view(tiles, np_queries, S).sum(dim=1) == 0).float().mean())


say(f"# python tools/radius_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, device ms between HIP "
    "events per call, median (min .. max) over the rounds; (a) coati_radius_count, (b) count + prefix sum + .item() + fill, "
    "(c) coati_search_topk k=1, (d) coati_search_topk k=128")
for N, E in LIBS:
    N = N // 64 if args.small else N
    g = torch.Generator(device=dev).manual_seed(E)
    index = EmbeddingIndex(E, metric="dot", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev))
    lib16 = index.vectors
    say(f"## library {N} x {E} bf16 = {lib16.numel() * 2 / 1e9:.3f} GB")
    for Q in QS:
        q16 = torch.randn(Q, E, generator=g, device=dev).to(torch.bfloat16)
        S = radius.default_slices(N, Q)
        inner = args.inner if Q < 1024 else max(1, args.inner // 3)
        tk = {}
        for k in (1, 128):
            Sk = _lib.lib().coati_search_slices(N, Q, k)
            tk[k] = (Sk, torch.empty(Q * Sk * k, device=dev), torch.empty(Q * Sk * k, dtype=torch.int32, device=dev), torch.empty(Q, k, device=dev),
                     torch.empty(Q, k, dtype=torch.long, device=dev))

        def topk(k):
            Sk, ps, pr, out_s, out_r = tk[k]
            _lib.call("coati_search_topk", ptr(lib16), N, E, ptr(index.bias), ptr(q16), Q, k, 1.0, Sk, ptr(ps), ptr(pr), ptr(out_s), ptr(out_r), stream())

        for hits in HITS:
            z = 1e3 if hits == 0 else float(torch.special.ndtri(torch.tensor(1.0 - hits / N, dtype=torch.float64)))
            thr = (q16.float().norm(dim=1) * z).contiguous()
            ops = radius.Operands(lib16, N, index.bias, q16, 1.0, None, 0, thr, None, S)
            fns = (ops.count, lambda: ops.search(1 << 28, "radius_bench"), lambda: topk(1), lambda: topk(128))
            for fn in fns:                                    # warm-up of every shape the timed window uses
                fn()
            torch.cuda.synchronize()
            t = [[], [], [], []]
            for _ in range(args.reps):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, inner))
            a, b, c, d = (statistics.median(x) for x in t)
            counts = ops.count()
            say(f"Q={Q:5d} S={S:3d} hits/query asked {hits:5d} counted {float(counts.sum()) / Q:9.1f}: (a) {spread(t[0])} ms   (b) {spread(t[1])} ms   "
                f"(c) {spread(t[2])} ms   (d) {spread(t[3])} ms   (a)/(c) {a / c:5.2f}   (b)/(d) {b / d:5.2f}   "
                f"fill workgroups that leave early {100 * early_share(counts, Q, S, 64 if E <= 256 else 32):5.1f} %")
    del index, lib16
    torch.cuda.empty_cache()

# ---- the self-join ------------------------------------------------------------------------------------------------------------------
N, E, chunk = (1 << 20) // (64 if args.small else 1), 256, 4096
g = torch.Generator(device=dev).manual_seed(7)
index = EmbeddingIndex(E, metric="cosine", device=dev)
for lo in range(0, N, 1 << 18):
    index.add(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev))


def self_join(triangle):
    total = 0
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        thr = torch.full((hi - lo,), 0.9, dtype=torch.float32, device=dev)
        row_hi = torch.arange(lo, hi, dtype=torch.int32, device=dev) if triangle else None
        ops = radius.Operands(index.vectors, N, index.bias, index.vectors[lo:hi], 1.0, None, 0, thr, row_hi, radius.self_join_slices(N, hi - lo))
        total += ops.search(1 << 28, "radius_bench")[1].numel()
    return total


say(f"## self-join of {N} x {E} bf16 (cosine >= 0.9, chunks of {chunk} queries, {radius.self_join_slices(N, chunk)} slices): count + fill per chunk")
found = [self_join(True), self_join(False)]                  # warm-up
torch.cuda.synchronize()
t = [[], []]
for _ in range(max(2, args.reps // 2)):
    for i, tri in enumerate((True, False)):
        t[i].append(timed(lambda: self_join(tri), 1))
say(f"triangle (row_hi[i] = i) {spread(t[0])} ms, {found[0]} pairs   square (no row bound) {spread(t[1])} ms, {found[1]} pairs   "
    f"triangle / square {statistics.median(t[0]) / statistics.median(t[1]):5.2f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
