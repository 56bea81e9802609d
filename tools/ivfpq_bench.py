"""The IVF-PQ search (coati_amd.ivfpq.IvfPqIndex) against the three indices it combines -- the bf16 IVF (coati_amd.ivf.IVFIndex), the fp8 IVF
(coati_amd.ivf8.Ivf8Index) and the exhaustive PQ (coati_amd.pq.PQIndex) -- by tools/ivf8_bench.py's method on its clustered libraries
(4 M rows x 256 with L = 2048 lists, 1 M rows x 256 with L = 1024; cosine, a mixture of 256 Gaussians, the queries fresh draws of it): in
one process, alternated round by round, device ms between HIP events, median (min .. max) over the rounds.  The three list indices hold
the SAME lists (from_ivf) and so the same probe tables.  Per library, Q in {1, 16, 64, 1024}, nprobe in {8, 32}, k = 10:
  (A)  ivfpq.search(q, k, nprobe): the coarse step, the probe table's inversion, coati_ivfpq_scan at R = min(oversample * k, k_max, 128),
       coati_ivf_merge and coati_search_rescore, behind the host-side preparation of the queries;
  (A1) ivfpq.search(..., rescore=False): stage 1 alone at k;
  (B)  ivf.search(q, k, nprobe);   (C) ivf8.search(q, k, nprobe);   (D) pq.search(q, k): every row, no lists.
Then recall@10 against index.search at oversample 2, 4 and 6 (and stage 1 alone) next to the bf16 IVF's and the flat PQ's, and the device
bytes each index holds beyond the source index.
python tools/ivfpq_bench.py [--reps 5] [--inner 10] [--iters 10] [--pq-iters 8] [--oversample 4] [--small] [--out profiles/ivfpq_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.fp8_index import R_MAX  # noqa: E402
from coati_amd.ivf8 import Ivf8Index  # noqa: E402
from coati_amd.ivfpq import IvfPqIndex, k_max  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--iters", type=int, default=10, help="k-means rounds of the lists")
ap.add_argument("--pq-iters", type=int, default=8, help="k-means rounds of the code books, flat and residual")
ap.add_argument("--oversample", type=int, default=4)
ap.add_argument("--small", action="store_true", help="1/64 of the rows and of the lists: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ivfpq_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256, 2048), (1 << 20, 256, 1024)]
QS, K, NPROBES = (1, 16, 64, 1024), 10, (8, 32)
COMPONENTS = 256
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:                                           # kept up to date: a run cut short leaves the cells it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(xs):
    return f"{statistics.median(xs):7.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def mixture(means, n, g):
    return means[torch.randint(0, means.shape[0], (n,), generator=g, device=dev)] + torch.randn(n, means.shape[1], generator=g, device=dev)


def recall(rows, exact):
    hit = (exact[:, :, None] == rows[:, None, :]).any(dim=2) & (exact >= 0)
    return float(hit.sum()) / max(int((exact >= 0).sum()), 1)


def held(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


say(f"# python tools/ivfpq_bench.py --reps {args.reps} --inner {args.inner} --iters {args.iters} --pq-iters {args.pq_iters} --oversample {args.oversample}"
    f"{' --small' if args.small else ''}: one MI355X, device ms between HIP events per call, median (min .. max) over the rounds; k = {K}; "
    "(A) ivfpq.search (two stages), (A1) ivfpq.search(rescore=False), (B) ivf.search, (C) ivf8.search (two stages), (D) pq.search (two stages, every row)")
for N, E, L in LIBS:
    if args.small:
        N, L = N // 64, max(L // 64, 4)
    g = torch.Generator(device=dev).manual_seed(E + L)
    means = torch.randn(min(COMPONENTS, N // 16), E, generator=g, device=dev)
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(mixture(means, min(1 << 18, N - lo), g))
    ivf = index.ivf(L, iters=args.iters, seed=0)
    ivf8 = Ivf8Index.from_ivf(ivf, index)
    torch.cuda.synchronize()
    t0 = time.time()
    ivfpq = IvfPqIndex.from_ivf(ivf, index, pq_iters=args.pq_iters)
    torch.cuda.synchronize()
    t1 = time.time()
    flat = index.pq(iters=args.pq_iters)
    torch.cuda.synchronize()
    sizes = ivf.sizes
    shared = held(ivf.ids, ivf.list_offsets, ivf.centres, ivf._inverse)
    say(f"## library {N} x {E}: the source index holds {held(index.vectors, index.bias) / 1e9:.3f} GB; L = {L} lists of {int(sizes.min())} .. {int(sizes.max())} rows "
        f"(median {int(sizes.median())}); residual code books fitted and rows coded in {t1 - t0:.2f} s (flat PQ: {time.time() - t1:.2f} s).  Device bytes "
        f"beyond the source index: IVFIndex {(held(ivf.vectors, ivf.bias) + shared) / 1e9:.3f} GB, Ivf8Index "
        f"{(held(ivf8.vectors8, ivf8.scales, ivf8.bias, ivf8._bias16) + shared) / 1e9:.3f} GB, IvfPqIndex "
        f"{(held(ivfpq.codes, ivfpq.bias, ivfpq.codebooks, ivfpq._bias16) + shared) / 1e9:.3f} GB (keep_rows=False: "
        f"{(held(ivfpq.codes, ivfpq.bias, ivfpq.codebooks) + shared) / 1e9:.3f} GB and no source index; {ivfpq.bytes_per_row()} B a row of codes, id and bias), "
        f"PQIndex {held(flat.codes, flat.bias, flat.codebooks, flat._bias16) / 1e9:.3f} GB")
    R = min(args.oversample * K, k_max(E), R_MAX)
    for nprobe in NPROBES:
        if nprobe > L:
            continue
        for Q in QS:
            q = mixture(means, Q, g)
            assert torch.equal(ivf.probe(q, nprobe), ivfpq.probe(q, nprobe)) and torch.equal(ivf.probe(q, nprobe), ivf8.probe(q, nprobe))
            fns = (lambda: ivfpq.search(q, K, nprobe=nprobe, oversample=args.oversample), lambda: ivfpq.search(q, K, nprobe=nprobe, rescore=False),
                   lambda: ivf.search(q, K, nprobe=nprobe), lambda: ivf8.search(q, K, nprobe=nprobe, oversample=args.oversample),
                   lambda: flat.search(q, K, oversample=args.oversample))
            for fn in fns:                                    # warm-up of every shape the timed window uses
                fn()
            torch.cuda.synchronize()
            t = [[] for _ in fns]
            for _ in range(args.reps):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, args.inner))
            A, A1, B, C, D = (statistics.median(x) for x in t)
            say(f"nprobe={nprobe:3d} Q={Q:5d} k={K:3d} R={R:3d} seg_rows={ivfpq.plan(Q, nprobe, R):5d}: (A) {spread(t[0])}   (A1) {spread(t[1])}   (B) {spread(t[2])}   "
                f"(C) {spread(t[3])}   (D) {spread(t[4])} ms   (A)/(B) {A / B:5.2f}   (A)/(C) {A / C:5.2f}   (A)/(D) {A / D:5.2f}   (A1)/(B) {A1 / B:5.2f}")
    # recall against the exact search; the list indices on the same probe tables (the coarse step is shared)
    Q = 1024
    q = mixture(means, Q, g)
    _, want = index.search(q, K)
    over = (2, 4, 6)
    rs = " / ".join(str(min(o * K, k_max(E), R_MAX)) for o in over)
    say(f"recall@{K} against index.search, {Q} queries: PQIndex (every row) stage 1 alone {recall(flat.search(q, K, rescore=False)[1], want):.4f}   two stages at "
        f"oversample 2 / 4 / 6: " + " / ".join(f"{recall(flat.search(q, K, oversample=o)[1], want):.4f}" for o in over))
    for nprobe in NPROBES:
        r16 = recall(ivf.search(q, K, nprobe=nprobe)[1], want)
        r8 = recall(ivf8.search(q, K, nprobe=nprobe, oversample=args.oversample)[1], want)
        r1 = recall(ivfpq.search(q, K, nprobe=nprobe, rescore=False)[1], want)
        two = [recall(ivfpq.search(q, K, nprobe=nprobe, oversample=o)[1], want) for o in over]
        say(f"recall@{K} against index.search, {Q} queries, nprobe={nprobe:3d}: IVFIndex {r16:.4f}   Ivf8Index (oversample {args.oversample}) {r8:.4f}   IvfPqIndex stage 1 "
            f"alone {r1:.4f}   two stages at oversample 2 / 4 / 6 (R = {rs}): " + " / ".join(f"{v:.4f}" for v in two))
    del index, ivf, ivf8, ivfpq, flat
    torch.cuda.empty_cache()
