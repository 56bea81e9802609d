"""The four-bit search (coati_search4_topk + coati_search_rescore through Fp4Index) against the exact search and the fp8 search, neither
of which it changes: per clustered library (4 M rows x 256 and 1 M rows x 512; 4096 Gaussian centres + 0.5-sigma noise, cosine), Q in
{1, 16, 64, 1024} and k in {10, 100}, in one process on the same library and alternated round by round,
  (a) EmbeddingIndex.search(q, k)                                the bf16 stream + the merge: the exact search;
  (b) Fp8Index.search(q, k)                                      its two stages at its default oversample (4);
  (c) Fp4Index.search(q, R, rescore=False)                       stage 1 alone at R = min(oversample * k, 128) candidates;
  (d) Fp4Index.search(q, k, oversample)                          the two stages.
All four are the classes' own calls, host-side preparation and quantisation of the queries included.  Device ms between HIP events
around --inner back-to-back calls, median and min .. max over --reps rounds.  Then recall@10 against the exact search on a clustered
library (1 M x 256, the same law, 1024 queries): stage 1 alone and the two stages at oversample 2, 4, 8, 12, fp4 next to fp8.
python tools/search4_bench.py [--reps 5] [--inner 10] [--oversample 8] [--small] [--out profiles/search4_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.fp8_index import R_MAX  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--oversample", type=int, default=8)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("search4_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256), (1 << 20, 512)]
QS, KS, C = (1, 16, 64, 1024), (10, 100), 4096
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


def clustered(E, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(C, E, generator=g, device=dev)
    return lambda n: centres[torch.randint(0, C, (n,), generator=g, device=dev)] + 0.5 * torch.randn(n, E, generator=g, device=dev)


def filled(N, E, draw):
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(draw(min(1 << 18, N - lo)))
    return index


def recall(want, rows):
    return 100 * sum(len(set(x) & set(y)) for x, y in zip(want.tolist(), rows.tolist())) / want.numel()


say(f"# python tools/search4_bench.py --reps {args.reps} --inner {args.inner} --oversample {args.oversample}{' --small' if args.small else ''}: one MI355X, "
    "device ms between HIP events per call, median (min .. max) over the rounds; (a) EmbeddingIndex.search, (b) Fp8Index.search (two stages, "
    "oversample 4), (c) Fp4Index stage 1 alone at R candidates, (d) Fp4Index.search (two stages)")
for N, E in LIBS:
    N = N // 64 if args.small else N
    draw = clustered(E, E)
    index = filled(N, E, draw)
    fp8, fp4 = index.fp8(), index.fp4()
    say(f"## library {N} x {E}, clustered, cosine: bf16 {N * (2 * E + 4) / 1e9:.3f} GB ({2 * E + 4} B a row), fp8 {N * (E + 8) / 1e9:.3f} GB ({E + 8} B), "
        f"fp4 {N * fp4.bytes_per_row() / 1e9:.3f} GB ({fp4.bytes_per_row()} B)")
    for Q in QS:
        q = draw(Q)
        for k in KS:
            R = min(args.oversample * k, R_MAX)
            fns = (lambda: index.search(q, k), lambda: fp8.search(q, k), lambda: fp4.search(q, R, rescore=False),
                   lambda: fp4.search(q, k, oversample=args.oversample))
            for fn in fns:                                    # warm-up of every shape the timed window uses
                fn()
            torch.cuda.synchronize()
            t = [[], [], [], []]
            for _ in range(args.reps):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, args.inner))
            a, b, c, d = (statistics.median(x) for x in t)
            want = index.search(q, k)[1]
            say(f"Q={Q:5d} k={k:3d} R={R:3d}: (a) {spread(t[0])} ms   (b) {spread(t[1])} ms   (c) {spread(t[2])} ms   (d) {spread(t[3])} ms   "
                f"(d)/(a) {d / a:5.2f}   (d)/(b) {d / b:5.2f}   (c)/(a) {c / a:5.2f}   recall@{k} of (b) {recall(want, fp8.search(q, k)[1]):.1f} %, of (d) "
                f"{recall(want, fp4.search(q, k, oversample=args.oversample)[1]):.1f} %")
    del index, fp8, fp4
    torch.cuda.empty_cache()

# recall on the clustered 1 M x 256 library, fp4 next to fp8
N, E, Q, k = (1 << 20) // (64 if args.small else 1), 256, 1024, 10
draw = clustered(E, 7)
index = filled(N, E, draw)
fp8, fp4 = index.fp8(), index.fp4()
q = draw(Q)
want = index.search(q, k)[1]
say(f"## recall@{k} against the exact search: {N} x {E} cosine, {C} centres + 0.5-sigma noise, {Q} queries of the same law")
say(f"stage 1 alone (rescore=False): fp4 {recall(want, fp4.search(q, k, rescore=False)[1]):.2f} %   fp8 {recall(want, fp8.search(q, k, rescore=False)[1]):.2f} %")
for over in (2, 4, 8, 12):
    say(f"two stages, oversample={over:2d} (R = {min(over * k, R_MAX):3d}): fp4 {recall(want, fp4.search(q, k, oversample=over)[1]):.2f} %   "
        f"fp8 {recall(want, fp8.search(q, k, oversample=over)[1]):.2f} %")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
