"""The IVF approximate search (coati_amd.ivf.IVFIndex) against the exact kernel it is built beside and against the memory system, by
tools/search_bench.py's method: in one process, alternated round by round, device ms between HIP events, median over the rounds.
Per library (4 M rows x 256 with L = 2048 lists, 1 M rows x 512 with L = 1024; bf16, cosine, a mixture of 256 Gaussians as wide as their means are
spread -- every component is cut into several lists, so a query's neighbours do cross list boundaries -- the queries fresh draws of the
same mixture), nprobe in {1, 8, 32}, Q in {1, 16, 64, 1024} and k in {10, 100}:
  (a) ivf.search(q, k, nprobe): the coarse step (coati_search_topk on the centres), the probe table's inversion in torch, coati_ivf_scan
      and coati_ivf_merge, behind the host-side preparation of the queries;   (a*) coati_ivf_scan + coati_ivf_merge alone, on a prepared
      probe table;
  (b) coati_search_topk on the same library, prepared buffers: the exact kernel, the thing to beat;
  (c) a device-to-device copy_ of as many bytes as the probed lists hold, every list counted once however many queries probe it: the
      floor of a scan that reads every wanted row once;
  recall@k: the share of (b)'s rows that (a) returns.
python tools/ivf_bench.py [--reps 5] [--inner 10] [--iters 10] [--small] [--out profiles/ivf_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd import ivf as ivf_mod  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex, prepare_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--iters", type=int, default=10, help="k-means rounds of the build")
ap.add_argument("--small", action="store_true", help="1/64 of the rows and of the lists: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ivf_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256, 2048), (1 << 20, 512, 1024)]
QS, KS, NPROBES = (1, 16, 64, 1024), (10, 100), (1, 8, 32)
COMPONENTS = 256
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


def mixture(means, n, g):
    return means[torch.randint(0, means.shape[0], (n,), generator=g, device=dev)] + torch.randn(n, means.shape[1], generator=g, device=dev)


def recall(rows, exact):
    hit = (exact[:, :, None] == rows[:, None, :]).any(dim=2) & (exact >= 0)
    return float(hit.sum()) / max(int((exact >= 0).sum()), 1)


say(f"# python tools/ivf_bench.py --reps {args.reps} --inner {args.inner} --iters {args.iters}{' --small' if args.small else ''}: one MI355X, device ms "
    "between HIP events per call, median (min .. max) over the rounds; (a) ivf.search, (a*) coati_ivf_scan + coati_ivf_merge alone, "
    "(b) coati_search_topk on the whole library, (c) copy_ of the probed lists' bytes (every list once)")
for N, E, L in LIBS:
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
    gb = index.vectors.numel() * 2 / 1e9
    say(f"## library {N} x {E} bf16 = {gb:.3f} GB, L = {L} lists of {int(sizes.min())} .. {int(sizes.max())} rows (median {int(sizes.median())}), "
        f"built in {time.time() - t0:.1f} s ({args.iters} k-means rounds)")
    lib16, src = index.vectors, ivf.vectors.reshape(-1)
    dst = torch.empty_like(src)
    for nprobe in NPROBES:
        if nprobe > L:
            continue
        for Q in QS:
            q = mixture(means, Q, g)
            _, q16 = prepare_queries(q, "cosine", E, dev)
            table = ivf.probe(q, nprobe)
            unique = torch.unique(table[table >= 0])
            wanted = int(sizes[unique].sum()) * E                                # bf16 elements of the lists at least one query probes
            pairs = int(sizes[table[table >= 0]].sum()) * E                      # ... counted once per query that probes them
            for k in KS:
                S = _lib.lib().coati_search_slices(N, Q, k)
                ps, pr = torch.empty(Q * S * k, device=dev), torch.empty(Q * S * k, dtype=torch.int32, device=dev)
                out_s, out_r = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.long, device=dev)
                seg_rows = ivf.plan(Q, nprobe, k)
                segs = max(1, -(-int(sizes.max()) // seg_rows))
                table32 = table.to(torch.int32).contiguous()
                pair_q, pair_off, item_off, pair_slot = ivf_mod.invert_probes(table32, sizes, seg_rows)
                P = Q * nprobe
                qs, qr = torch.empty(P * segs * k, device=dev), torch.empty(P * segs * k, dtype=torch.int32, device=dev)
                iv_s, iv_r = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.long, device=dev)

                def exact():
                    _lib.call("coati_search_topk", ptr(lib16), N, E, ptr(index.bias), ptr(q16), Q, k, 1.0, S, ptr(ps), ptr(pr), ptr(out_s),
                              ptr(out_r), stream())

                def kernels():
                    _lib.call("coati_ivf_scan", ptr(ivf.vectors), ptr(ivf.ids), ptr(ivf.bias), ptr(ivf.list_offsets), ivf.vectors.shape[0], E, L,
                              ptr(q16), Q, ptr(pair_q), ptr(pair_off), ptr(item_off), P, k, 1.0, seg_rows, segs, ptr(qs), ptr(qr), 0, stream())
                    _lib.call("coati_ivf_merge", ptr(qs), ptr(qr), ptr(table32), ptr(pair_slot), P, ptr(ivf.list_offsets), L, Q, nprobe, k,
                              seg_rows, segs, ptr(iv_s), ptr(iv_r), stream())

                fns = (lambda: ivf.search(q, k, nprobe=nprobe), kernels, exact, lambda: dst[:wanted].copy_(src[:wanted]))
                inner = (args.inner, args.inner, 2 if Q >= 64 else args.inner, args.inner)
                for fn in fns:                                    # warm-up of every shape the timed window uses
                    fn()
                torch.cuda.synchronize()
                t = [[], [], [], []]
                for _ in range(args.reps):
                    for i, fn in enumerate(fns):
                        t[i].append(timed(fn, inner[i]))
                a, a1, b, c = (statistics.median(x) for x in t)
                rows_a = ivf.search(q, k, nprobe=nprobe)[1]
                assert torch.equal(rows_a, iv_r)
                say(f"nprobe={nprobe:3d} Q={Q:5d} k={k:3d} seg_rows={seg_rows:5d}: (a) {spread(t[0])} ms   (a*) {spread(t[1])} ms   (b) {spread(t[2])} ms   "
                    f"(c) {spread(t[3])} ms   (b)/(a) {b / a:7.2f}   (b)/(a*) {b / a1:7.2f}   (a*)/(c) {a1 / c:6.2f}   lists' bytes {wanted * 2 / 1e6:8.1f} MB "
                    f"once, {pairs * 2 / 1e6:8.1f} MB per pair   recall@{k} {recall(rows_a, out_r):.4f}")
    del index, ivf, lib16, src, dst
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
