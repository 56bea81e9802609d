"""The radius search over inverted lists (IVFIndex.radius_search / near_duplicates, coati_amd.ivf_radius) against the exact radius search
it approximates (EmbeddingIndex.radius_search / near_duplicates, unchanged by it), in one process, alternated round by round.  Both end
in a synchronisation of their own (the .item() between the passes), so a call is timed on the host clock between two device
synchronisations; median (min .. max) over the rounds.
Per library (clustered as tools/ivf_bench.py's: bf16, cosine, a mixture of 256 Gaussians as wide as their means are spread, the queries
fresh draws of the mixture; L lists by k-means):
  radius_search at Q in {1, 64, 1024} and nprobe in {8, 32}, the threshold of a query being its exact 100th best score, so the exact
      answer has about 100 hits per query:   (a) ivf.radius_search   (b) index.radius_search   found = (a)'s hits / (b)'s;
  near_duplicates at nprobe in {1, 8}, the threshold being the median 10th best score of 256 stored rows against the library:
      (a) ivf.near_duplicates   (b) index.near_duplicates   found = (a)'s pairs / (b)'s.
python tools/ivf_radius_bench.py [--rows 1048576,4194304] [--reps 5] [--join-reps 2] [--iters 10] [--small] [--out profiles/ivf_radius_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1048576,4194304")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--join-reps", type=int, default=2)
ap.add_argument("--iters", type=int, default=10, help="k-means rounds of the build")
ap.add_argument("--small", action="store_true", help="1/64 of the rows and of the lists: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ivf_radius_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, COMPONENTS = 256, 256
QS, NPROBES, JOIN_NPROBES = (1, 64, 1024), (8, 32), (1, 8)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def mixture(means, n, g):
    return means[torch.randint(0, means.shape[0], (n,), generator=g, device=dev)] + torch.randn(n, means.shape[1], generator=g, device=dev)


def alternated(fns, reps):
    """every function once per round, round by round, after one warm-up call each: (times per function, the last results)"""
    out = [fn() for fn in fns]
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms, out[i] = timed(fn)
            t[i].append(ms)
    return t, out


say(f"# python tools/ivf_radius_bench.py --rows {args.rows} --reps {args.reps} --join-reps {args.join_reps} --iters {args.iters}"
    f"{' --small' if args.small else ''}: one MI355X, host ms per call between device synchronisations, median (min .. max) over the rounds, "
    "the two forms alternated; (a) the IVFIndex method, (b) the EmbeddingIndex method on the same rows; found = (a)'s results / (b)'s")
for N in (int(v) for v in args.rows.split(",")):
    L = N // 2048
    if args.small:
        N, L = N // 64, max(L // 64, 4)
    g = torch.Generator(device=dev).manual_seed(E)
    means = torch.randn(min(COMPONENTS, N // 16), E, generator=g, device=dev)
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(mixture(means, min(1 << 18, N - lo), g))
    torch.cuda.synchronize()
    t0 = time.time()
    ivf = index.ivf(L, iters=args.iters, seed=0)
    torch.cuda.synchronize()
    sizes = ivf.sizes
    say(f"## library {N} x {E} bf16 = {index.vectors.numel() * 2 / 1e9:.3f} GB, L = {L} lists of {int(sizes.min())} .. {int(sizes.max())} rows "
        f"(median {int(sizes.median())}), built in {time.time() - t0:.1f} s ({args.iters} k-means rounds)")
    for Q in QS:
        q = mixture(means, Q, g)
        thr = index.search(q, 100)[0][:, 99].clone()
        for nprobe in NPROBES:
            t, out = alternated((lambda: ivf.radius_search(q, thr, nprobe=nprobe), lambda: index.radius_search(q, thr),
                                 lambda: ivf.radius_count(q, thr, nprobe=nprobe), lambda: index.radius_count(q, thr)), args.reps)
            a, b = statistics.median(t[0]), statistics.median(t[1])
            found, exact = out[0][1].numel(), out[1][1].numel()
            assert found <= exact and int(out[2].sum()) == found and int(out[3].sum()) == exact
            say(f"radius_search Q={Q:5d} nprobe={nprobe:3d} seg_rows={ivf.plan(Q, nprobe, 1):5d}: (a) {spread(t[0])} ms   (b) {spread(t[1])} ms   (b)/(a) {b / a:6.2f}   "
                f"count alone (a) {spread(t[2])} ms   (b) {spread(t[3])} ms   found {found} of {exact} = {found / max(exact, 1):.4f}")
    sample = index.vectors[torch.randint(0, N, (256,), generator=g, device=dev)].float()
    thr = float(index.search(sample, 11)[0][:, 10].median())
    # one round = the IVF join at every nprobe, then the exact join once
    t, out = alternated([lambda n=n: ivf.near_duplicates(thr, nprobe=n) for n in JOIN_NPROBES] + [lambda: index.near_duplicates(thr)], args.join_reps)
    b, exact = statistics.median(t[-1]), out[-1][1].numel()
    for i, nprobe in enumerate(JOIN_NPROBES):
        a, found = statistics.median(t[i]), out[i][1].numel()
        assert found <= exact
        say(f"near_duplicates cosine >= {thr:.4f} nprobe={nprobe:3d}: (a) {spread(t[i])} ms   (b) {spread(t[-1])} ms   (b)/(a) {b / a:6.2f}   "
            f"found {found} of {exact} pairs = {found / max(exact, 1):.4f}")
    del out
    del index, ivf
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
