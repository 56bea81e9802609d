"""Embedding maps (coati_amd/tsne.py, include/coati_tsne.h): what a map costs.  Per library size (10 k, 100 k and 1 M rows x 64, a mixture
of 64 Gaussians, cosine, perplexity 30, k = 90), in one process:
  (g)  the kNN graph (EmbeddingIndex.knn_graph: the search kernel on the stored rows), (p) coati_tsne_affinities, (j) joint() in torch;
  (r)  coati_tsne_repulsion on the map as it stands after --settle iterations, (s) coati_tsne_step, (z) the torch glue of an iteration
       (z.sum in float64 and its cast), (i) a whole iteration of layout()'s loop; pairs / s = N (N - 1) / (r).
The repulsion's pair loop is 50 VALU instructions per 8 pairs in the ISA (per lane: 8 v_pk_add_f32 for the 16 differences, 16 v_fma_f32
for 1 + |d|^2, 8 v_rcp_f32, 4 v_pk_mul_f32, 4 v_pk_add_f32, 8 v_pk_fma_f32, 2 v_mov_b32) = 6.25 a pair, and 13 flops a pair; the rate is
given as flops against the 157.3 TF f32 vector peak and as instruction issue against 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz, a v_rcp_f32
counted as two issue slots (8 cycles against 4).
  (k)  with --sklearn: sklearn.manifold.TSNE(method="exact", init="random", learning_rate=100) on the host at 512, 1024, 2048, ... rows
       up to the largest size that fits a minute (a fit is O(N^2): the next size is not tried once 4 x the last time exceeds it), next to index.tsne() -- graph, affinities and 1000 iterations -- on the same rows.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds.
    python tools/tsne_bench.py [--reps 5] [--inner 3] [--sizes 10000,100000,1000000] [--sklearn] [--out profiles/tsne_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import tsne  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--sizes", default="10000,100000,1000000")
ap.add_argument("--settle", type=int, default=20, help="iterations before the timed ones (the map leaves its 1e-4 start)")
ap.add_argument("--sklearn", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tsne_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, PERPLEXITY, K = 64, 30.0, 90
PEAK_TF, PEAK_ISSUE = 157.3, 256 * 4 * 32 * 2.4e9
lines = []
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()


def say(s):
    """a result line: printed, and appended to --out at once (a long run leaves what it has measured)"""
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")


def stage(s):
    print(f"  .. {s}", flush=True)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def mixture(n, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(64, E, generator=g)
    return centres[torch.arange(n) % 64] + 0.5 * torch.randn(n, E, generator=g)


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


say(f"# python tools/tsne_bench.py --reps {args.reps} --inner {args.inner} --sizes {args.sizes}{' --sklearn' if args.sklearn else ''}: one MI355X; "
    f"rows x {E}, cosine, perplexity {PERPLEXITY:g}, k = {K}; (g) (p) (j) wall ms of one call after a warm-up; (r) (s) (z) (i) device ms per call, "
    "median (min .. max) over the rounds")
for N in [int(s) for s in args.sizes.split(",") if s]:
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    index.add(mixture(N, N))
    index.knn_graph(K, chunk=4096) if N <= 100000 else None                        # warm-up where it is cheap
    (rows, nbr, d2), t_graph = once(lambda: index.knn_graph(K))
    stage(f"N={N}: kNN graph {t_graph:.0f} ms")
    tsne.affinities(d2[:1024], nbr[:1024], PERPLEXITY)
    p, t_aff = once(lambda: tsne.affinities(d2, nbr, PERPLEXITY))
    (offsets, cols, vals), t_joint = once(lambda: tsne.joint(nbr, p))
    del nbr, d2, p
    stage(f"affinities {t_aff:.1f} ms, joint {t_joint:.1f} ms")
    settled = tsne.layout(offsets, cols, vals, N, iters=args.settle, kl_every=args.settle).y
    torch.cuda.synchronize()
    stage(f"{args.settle} iterations done")
    other, update, gains = torch.empty_like(settled), torch.zeros_like(settled), torch.ones_like(settled)
    rep, z = torch.empty_like(settled), torch.empty(N, device=dev)
    part = tsne.part_for(N, dev)
    state = {"zsum": torch.ones(1, device=dev)}
    rate = max(N / 12.0 / 4.0, 50.0)

    def repulsion():
        tsne.repulsion(settled, part, out=(rep, z))

    def glue():
        state["zsum"] = z.sum(dtype=torch.float64).float().reshape(1)

    def step():
        tsne.step(settled, rep, state["zsum"], offsets, cols, vals, update, gains, other, exaggeration=12.0, momentum=0.5, lr=rate)

    def iteration():
        repulsion()
        glue()
        step()

    fns = (repulsion, glue, step, iteration)
    inner = args.inner if N < 500000 else 1
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.reps if N < 500000 else min(args.reps, 3)):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, inner))
    r = statistics.median(t[0])
    pairs = N * (N - 1) / (r * 1e-3)
    say(f"N={N:8d}: nnz {int(offsets[-1])}, repulsion workspace {'%.1f MB' % (part.numel() * 4 / 1e6) if part is not None else 'none'}   (g) {t_graph:10.1f} ms   "
        f"(p) {t_aff:8.2f} ms   (j) {t_joint:8.2f} ms   (r) {spread(t[0])} ms   (s) {spread(t[2])} ms   (z) {spread(t[1])} ms   (i) {spread(t[3])} ms   "
        f"pairs/s {pairs:.3e}   {pairs * 13 / 1e12:6.1f} TF = {100 * pairs * 13 / 1e12 / PEAK_TF:4.1f} % of {PEAK_TF} TF   "
        f"issue {100 * pairs * 7.25 / PEAK_ISSUE:4.1f} % of peak (6.25 instructions a pair, v_rcp_f32 counted twice)")
    del index, settled, other, update, gains, rep, z, part, offsets, cols, vals
    torch.cuda.empty_cache()

if args.sklearn:
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        TSNE = None
        say("(k) sklearn is not installed: no host baseline")
    n = 512
    while TSNE is not None:
        x = mixture(n, n)
        x = x / x.norm(dim=1, keepdim=True)
        t0 = time.perf_counter()
        model = TSNE(n_components=2, learning_rate=100, init="random", method="exact", random_state=0)
        model.fit_transform(x.numpy())
        host = time.perf_counter() - t0
        stage(f"sklearn N={n}: {host:.1f} s")
        index = EmbeddingIndex(E, metric="cosine", device=dev)
        index.add(x)
        index.tsne(iters=10)
        res, ours = once(lambda: index.tsne(perplexity=PERPLEXITY, iters=1000, lr=100.0))
        say(f"(k) N={n:6d}: sklearn exact {host:7.1f} s ({model.n_iter_} iterations, KL {model.kl_divergence_:.4f} of the dense P)   "
            f"index.tsne 1000 iterations {ours / 1e3:7.3f} s (KL {res.kl:.4f} of P on {min(n - 1, K)} neighbours)   {host / (ours / 1e3):7.1f} x")
        if 4 * host > 60.0:
            break
        n *= 2
