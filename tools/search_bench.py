"""The embedding-library search (coati_search_topk through EmbeddingIndex.search) against what torch offers and against the memory
system: per library (4 M rows x 256 and 1 M rows x 512, bf16, Gaussian), Q in {1, 16, 64, 1024} and k in {10, 100}, in one process and
alternated round by round,
  (a) coati_search_topk on prepared buffers               the streaming kernel + the merge;  (a') index.search(q, k): the same behind
      the host-side preparation of the queries and the result tensors;
  (b) (q @ lib.T).topk(k) over library chunks that keep the score matrix under 2 GB, merged by a second topk   (bf16 GEMM of the
      vendor library: its scores are rounded to bf16, so its order is approximate where (a)'s is exact);
  (c) a device-to-device copy_ of the library's bytes       the bandwidth yardstick: it reads the library once (and writes it once).
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds; library GB/s = the library's
bytes over the time.   python tools/search_bench.py [--reps 5] [--inner 10] [--small] [--out profiles/search_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("search_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256), (1 << 20, 512)]
QS, KS = (1, 16, 64, 1024), (10, 100)
SCORE_BYTES = 2 << 30
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


def torch_search(lib16, q16, k):
    N, Q = lib16.shape[0], q16.shape[0]
    chunk = max(k, min(N, SCORE_BYTES // (4 * Q)))
    vals, idxs = [], []
    for lo in range(0, N, chunk):
        v, i = (q16 @ lib16[lo:lo + chunk].T).topk(min(k, N - lo), dim=1)
        vals.append(v)
        idxs.append(i + lo)
    if len(vals) == 1:
        return vals[0], idxs[0]
    v, j = torch.cat(vals, dim=1).topk(k, dim=1)
    return v, torch.cat(idxs, dim=1).gather(1, j)


def spread(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):.3f} .. {max(xs):.3f})"


say(f"# python tools/search_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, device ms between HIP "
    "events per call, median (min .. max) over the rounds; (a) coati_search_topk, (a') index.search, (b) torch (q @ lib.T).topk per <= 2 GB of scores, (c) copy_ of the library")
for N, E in LIBS:
    N = N // 64 if args.small else N
    g = torch.Generator(device=dev).manual_seed(E)
    index = EmbeddingIndex(E, metric="dot", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev))
    lib16 = index.vectors
    dst = torch.empty_like(lib16)
    gb = lib16.numel() * 2 / 1e9
    say(f"## library {N} x {E} bf16 = {gb:.3f} GB")
    for Q in QS:
        q = torch.randn(Q, E, generator=g, device=dev)
        q16 = q.to(torch.bfloat16)
        for k in KS:
            S = _lib.lib().coati_search_slices(N, Q, k)
            ps, pr = torch.empty(Q * S * k, device=dev), torch.empty(Q * S * k, dtype=torch.int32, device=dev)
            out_s, out_r = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.long, device=dev)

            def raw():
                _lib.call("coati_search_topk", ptr(lib16), N, E, ptr(index.bias), ptr(q16), Q, k, 1.0, S, ptr(ps), ptr(pr), ptr(out_s), ptr(out_r),
                          stream())

            fns = (raw, lambda: torch_search(lib16, q16, k), lambda: dst.copy_(lib16), lambda: index.search(q, k))
            inner = (args.inner, 1 if Q >= 64 else args.inner, args.inner, args.inner)
            for fn in fns:                                    # warm-up of every shape the timed window uses
                fn()
            torch.cuda.synchronize()
            t = [[], [], [], []]
            for _ in range(args.reps):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, inner[i]))
            a, b, c, a2 = (statistics.median(x) for x in t)
            rows_a, rows_b = index.search(q, k)[1], torch_search(lib16, q16, k)[1]
            assert torch.equal(rows_a, out_r)
            same = sum(len(set(x) & set(y)) for x, y in zip(rows_a.tolist(), rows_b.tolist())) / (Q * k)
            say(f"Q={Q:5d} k={k:3d} S={S:3d}: (a) {spread(t[0])} ms = {gb / a * 1e3:7.1f} GB/s   (b) {spread(t[1])} ms   (c) {spread(t[2])} ms = "
                f"{gb / c * 1e3:7.1f} GB/s   (a)/(c) {a / c:6.2f}   (a)/(b) {a / b:6.3f}   (a') {a2:8.3f} ms   rows shared with (b) {100 * same:.1f} %")
    del index, lib16, dst
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
