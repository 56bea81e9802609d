"""One Lloyd round over an embedding library (coati_cluster_assign + coati_cluster_sums, coati_amd/cluster.py) against what the library
offered before them and against the memory system: per shape (4 M rows x 256 with K in {64, 1024, 4096}, 1 M rows x 512 with K = 1024; bf16,
unit Gaussian rows, spherical k-means), in one process and alternated round by round,
  (a)  one Lloyd round: assign + the stable sort and the counts + sums + the mean;   (a1), (a2): the two kernels alone;
  (b)  the same round in torch: a bf16 x @ c.T over library chunks that keep the scores under 2 GB (the vendor GEMM rounds them to bf16, so
       its argmax is approximate where (a)'s is exact) + argmax + index_add_ of an f32 copy of the rows (float atomics) + the mean;
  (b1) coati_search_topk with the roles swapped -- the centres as the library, the rows as queries, k = 1 -- as the assignment only;
  (c)  a device-to-device copy_ of the library's bytes: the bandwidth yardstick.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds.
    python tools/cluster_bench.py [--reps 5] [--inner 3] [--small] [--out profiles/cluster_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib, cluster  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("cluster_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
SHAPES = [(4 << 20, 256, 64), (4 << 20, 256, 1024), (4 << 20, 256, 4096), (1 << 20, 512, 1024)]
SCORE_BYTES = 2 << 30
QUERY_CHUNK = 1 << 20
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


def normalised(m):
    return m / m.norm(dim=1, keepdim=True).clamp_min(1e-30)


say(f"# python tools/cluster_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, device ms between HIP "
    "events per call, median (min .. max) over the rounds; (a) a Lloyd round, (a1) coati_cluster_assign, (a2) coati_cluster_sums, (b) the round in "
    "torch (bf16 GEMM per <= 2 GB of scores + argmax + index_add_ of f32 rows), (b1) coati_search_topk k = 1 with the rows as queries, (c) copy_ of the library")
ch = cluster.chunk_rows()
lib16 = None
for N, E, K in SHAPES:
    N = N // 64 if args.small else N
    if lib16 is None or lib16.shape != (N, E):
        del lib16
        torch.cuda.empty_cache()
        g = torch.Generator(device=dev).manual_seed(E)
        lib16 = torch.cat([normalised(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev)).to(torch.bfloat16) for lo in range(0, N, 1 << 18)])
        lib32, dst = lib16.float(), torch.empty_like(lib16)
        gb = lib16.numel() * 2 / 1e9
        say(f"## library {N} x {E} bf16 = {gb:.3f} GB")
    centres = lib32[torch.randperm(N, generator=torch.Generator().manual_seed(K))[:K].to(dev)].clone()
    c16 = centres.to(torch.bfloat16).contiguous()
    part = torch.empty((N // ch + K) * E, device=dev)
    state = {}

    def assign_only():
        state["assign"], state["best"] = cluster.assign_call(lib16, None, c16)

    def inverted():
        order, sizes = cluster.sorted_order(state["assign"], K)
        state["sizes"], state["order32"] = sizes, order.to(torch.int32)
        state["offsets"], state["item_off"] = cluster.item_table(sizes, ch)

    def sums_only():
        state["sums"] = cluster.sums_call(lib16, state["order32"], state["offsets"], state["item_off"], part)

    def ours():
        assign_only()
        inverted()
        sums_only()
        mean = normalised(state["sums"] / state["sizes"].clamp_min(1).float()[:, None])
        state["centres"] = torch.where((state["sizes"] > 0)[:, None], mean, centres)

    def torch_round():
        chunk = max(1, min(N, SCORE_BYTES // (2 * K)))
        a = torch.cat([(lib16[lo:lo + chunk] @ c16.T).argmax(dim=1) for lo in range(0, N, chunk)])
        sums = torch.zeros(K, E, device=dev).index_add_(0, a, lib32)
        sizes = torch.bincount(a, minlength=K)
        mean = normalised(sums / sizes.clamp_min(1).float()[:, None])
        state["t_assign"], state["t_centres"] = a, torch.where((sizes > 0)[:, None], mean, centres)

    qc = min(N, QUERY_CHUNK)
    S = _lib.lib().coati_search_slices(K, qc, 1)
    ps, pr = torch.empty(qc * S, device=dev), torch.empty(qc * S, dtype=torch.int32, device=dev)
    out_s, out_r = torch.empty(N, 1, device=dev), torch.empty(N, 1, dtype=torch.long, device=dev)

    def swapped_search():
        for lo in range(0, N, qc):
            n = min(qc, N - lo)
            _lib.call("coati_search_topk", ptr(c16), K, E, None, ptr(lib16[lo:lo + n]), n, 1, 1.0, S, ptr(ps), ptr(pr), ptr(out_s[lo:lo + n]),
                      ptr(out_r[lo:lo + n]), stream())

    fns = (ours, assign_only, sums_only, torch_round, swapped_search, lambda: dst.copy_(lib16))
    for fn in fns:                                    # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.reps):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, args.inner))
    a, a1, a2, b, b1, c = (statistics.median(x) for x in t)
    ours()
    assert torch.equal(out_r[:, 0], state["assign"].long())                      # the swapped search is the same exact assignment
    same = float((state["t_assign"] == state["assign"].long()).float().mean())
    say(f"K={K:5d}: (a) {spread(t[0])} ms   (a1) {spread(t[1])} ms = {gb / a1 * 1e3:7.1f} GB/s   (a2) {spread(t[2])} ms = {gb / a2 * 1e3:7.1f} GB/s   "
        f"(b) {spread(t[3])} ms   (b1) {spread(t[4])} ms   (c) {spread(t[5])} ms = {gb / c * 1e3:7.1f} GB/s   (a)/(b) {a / b:6.3f}   "
        f"(a1)/(b1) {a1 / b1:6.3f}   (a1)/(c) {a1 / c:6.2f}   rows assigned as (b) {100 * same:.2f} %   empty clusters {int((state['sizes'] == 0).sum())}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
