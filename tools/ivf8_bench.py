"""The IVF search over fp8 lists (coati_amd.ivf8.Ivf8Index) against the bf16 IVF search it halves the bytes of (coati_amd.ivf.IVFIndex),
by tools/ivf_bench.py's method and on its two libraries (4 M rows x 256 with L = 2048 lists, 1 M rows x 512 with L = 1024; cosine, a
mixture of 256 Gaussians, the queries fresh draws of it): in one process, alternated round by round, device ms between HIP events, median
(min .. max) over the rounds.  Both indices hold the SAME lists (Ivf8Index.from_ivf) and every cell gives both the same probe table.
Per library, Q in {1, 16, 64, 1024}, nprobe in {8, 32} and k in {10, 100}:
  (A)  ivf8.search(q, k, nprobe): the coarse step, the queries' quantisation, the probe table's inversion, coati_ivf8_scan at
       R = min(oversample * k, 128), coati_ivf_merge and coati_search_rescore, behind the host-side preparation of the queries;
  (A1) ivf8.search(..., rescore=False): stage 1 alone at k;
  (A*) coati_ivf8_scan + coati_ivf_merge alone at R, on a prepared probe table and prepared quantised queries;
  (B)  ivf.search(q, k, nprobe);      (B*) coati_ivf_scan + coati_ivf_merge alone at k.
Then recall@k of both indices against index.search (the fp8 one at oversample 2, 4 and 8, and stage 1 alone), and the device bytes each
index holds beyond the source index.
python tools/ivf8_bench.py [--reps 5] [--inner 10] [--iters 10] [--oversample 4] [--small] [--out profiles/ivf8_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd import ivf as ivf_mod  # noqa: E402
from coati_amd.fp8_index import R_MAX, quantise_device  # noqa: E402
from coati_amd.ivf8 import Ivf8Index  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex, prepare_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--iters", type=int, default=10, help="k-means rounds of the build")
ap.add_argument("--oversample", type=int, default=4)
ap.add_argument("--small", action="store_true", help="1/64 of the rows and of the lists: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ivf8_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256, 2048), (1 << 20, 512, 1024)]
QS, KS, NPROBES = (1, 16, 64, 1024), (10, 100), (8, 32)
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


say(f"# python tools/ivf8_bench.py --reps {args.reps} --inner {args.inner} --iters {args.iters} --oversample {args.oversample}{' --small' if args.small else ''}: "
    "one MI355X, device ms between HIP events per call, median (min .. max) over the rounds; (A) ivf8.search (two stages), (A1) ivf8.search(rescore=False), "
    "(A*) coati_ivf8_scan + coati_ivf_merge alone at R candidates, (B) ivf.search, (B*) coati_ivf_scan + coati_ivf_merge alone at k")
for N, E, L in LIBS:
    if args.small:
        N, L = N // 64, max(L // 64, 4)
    g = torch.Generator(device=dev).manual_seed(E)
    means = torch.randn(min(COMPONENTS, N // 16), E, generator=g, device=dev)
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(mixture(means, min(1 << 18, N - lo), g))
    ivf = index.ivf(L, iters=args.iters, seed=0)
    torch.cuda.synchronize()
    t0 = time.time()
    ivf8 = Ivf8Index.from_ivf(ivf, index)
    torch.cuda.synchronize()
    sizes = ivf.sizes
    M = ivf.vectors.shape[0]
    shared = held(ivf.ids, ivf.list_offsets, ivf.centres, ivf._inverse)
    say(f"## library {N} x {E}: the source index holds {held(index.vectors, index.bias) / 1e9:.3f} GB; L = {L} lists of {int(sizes.min())} .. {int(sizes.max())} rows "
        f"(median {int(sizes.median())}); quantised in {time.time() - t0:.2f} s.  Device bytes beyond the source index: IVFIndex "
        f"{(held(ivf.vectors, ivf.bias) + shared) / 1e9:.3f} GB, Ivf8Index {(held(ivf8.vectors8, ivf8.scales, ivf8.bias, ivf8._bias16) + shared) / 1e9:.3f} GB "
        f"(keep_rows=False: {(held(ivf8.vectors8, ivf8.scales, ivf8.bias) + shared) / 1e9:.3f} GB and no source index)")
    for nprobe in NPROBES:
        if nprobe > L:
            continue
        for Q in QS:
            q = mixture(means, Q, g)
            _, q16 = prepare_queries(q, "cosine", E, dev)
            q8, qscale = quantise_device(q16)
            table = ivf.probe(q, nprobe)
            assert torch.equal(table, ivf8.probe(q, nprobe))
            table32 = table.to(torch.int32).contiguous()
            P = Q * nprobe
            for k in KS:
                R = min(args.oversample * k, R_MAX)
                plans = []
                for kk in (R, k):
                    seg_rows = ivf.plan(Q, nprobe, kk)
                    segs = max(1, -(-int(sizes.max()) // seg_rows))
                    tabs = ivf_mod.invert_probes(table32, sizes, seg_rows)
                    plans.append((kk, seg_rows, segs, tabs, torch.empty(P * segs * kk, device=dev), torch.empty(P * segs * kk, dtype=torch.int32, device=dev),
                                  torch.empty(Q, kk, device=dev), torch.empty(Q, kk, dtype=torch.long, device=dev)))

                def merge(kk, seg_rows, segs, tabs, ps, pr, out_s, out_r):
                    _lib.call("coati_ivf_merge", ptr(ps), ptr(pr), ptr(table32), ptr(tabs[3]), P, ptr(ivf.list_offsets), L, Q, nprobe, kk, seg_rows, segs,
                              ptr(out_s), ptr(out_r), stream())

                def kernels8():
                    kk, seg_rows, segs, tabs, ps, pr, out_s, out_r = plans[0]
                    _lib.call("coati_ivf8_scan", ptr(ivf8.vectors8), ptr(ivf8.scales), ptr(ivf8.ids), ptr(ivf8.bias), ptr(ivf8.list_offsets), M, E, L,
                              ptr(q8), ptr(qscale), Q, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), P, kk, 1.0, seg_rows, segs, ptr(ps), ptr(pr), 0, stream())
                    merge(*plans[0])

                def kernels16():
                    kk, seg_rows, segs, tabs, ps, pr, out_s, out_r = plans[1]
                    _lib.call("coati_ivf_scan", ptr(ivf.vectors), ptr(ivf.ids), ptr(ivf.bias), ptr(ivf.list_offsets), M, E, L, ptr(q16), Q, ptr(tabs[0]),
                              ptr(tabs[1]), ptr(tabs[2]), P, kk, 1.0, seg_rows, segs, ptr(ps), ptr(pr), 0, stream())
                    merge(*plans[1])

                fns = (lambda: ivf8.search(q, k, nprobe=nprobe, oversample=args.oversample), lambda: ivf8.search(q, k, nprobe=nprobe, rescore=False),
                       kernels8, lambda: ivf.search(q, k, nprobe=nprobe), kernels16)
                for fn in fns:                                    # warm-up of every shape the timed window uses
                    fn()
                torch.cuda.synchronize()
                t = [[] for _ in fns]
                for _ in range(args.reps):
                    for i, fn in enumerate(fns):
                        t[i].append(timed(fn, args.inner))
                A, A1, As, B, Bs = (statistics.median(x) for x in t)
                assert torch.equal(ivf.search(q, k, nprobe=nprobe)[1], plans[1][7])
                say(f"nprobe={nprobe:3d} Q={Q:5d} k={k:3d} R={R:3d} seg_rows={plans[0][1]:5d}/{plans[1][1]:5d}: (A) {spread(t[0])}   (A1) {spread(t[1])}   "
                    f"(A*) {spread(t[2])}   (B) {spread(t[3])}   (B*) {spread(t[4])} ms   (A)/(B) {A / B:5.2f}   (A1)/(B) {A1 / B:5.2f}   (A*)/(B*) {As / Bs:5.2f}")
    # recall against the exact search, both indices on the same probe tables (the coarse step is shared)
    Q = 1024
    q = mixture(means, Q, g)
    for k in KS:
        _, want = index.search(q, k)
        for nprobe in NPROBES:
            r16 = recall(ivf.search(q, k, nprobe=nprobe)[1], want)
            r1 = recall(ivf8.search(q, k, nprobe=nprobe, rescore=False)[1], want)
            two = [recall(ivf8.search(q, k, nprobe=nprobe, oversample=o)[1], want) for o in (2, 4, 8)]
            say(f"recall@{k} against index.search, {Q} queries, nprobe={nprobe:3d}: IVFIndex {r16:.4f}   Ivf8Index stage 1 alone {r1:.4f}   two stages at "
                f"oversample 2 / 4 / 8 (R = {min(2 * k, R_MAX)} / {min(4 * k, R_MAX)} / {min(8 * k, R_MAX)}): {two[0]:.4f} / {two[1]:.4f} / {two[2]:.4f}")
    del index, ivf, ivf8
    torch.cuda.empty_cache()
