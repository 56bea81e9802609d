"""The fused GP-head kernel (coati_head_gp, csrc/gp.hip) against the deterministic head it extends (coati_head_eval, csrc/screen.hip) on the
same bf16 library: E = F = 256, D = 4, P = 1, M = 60 inducing points (padded to 64) on Gaussian unit rows, N = 1 M, in one process and
alternated round by round,
  (a) coati_head_eval on the library's rows                 the extractor and its linear last layer: [N, 1] floats written;
  (b) coati_head_gp on the same rows                        the same forward, then mean [N, 1] and var [N];
  (c) coati_head_gp with the linear layer as well           (b) plus (a)'s output from the same pass;
  (d) index.screen(gp, 10, acquisition="ucb")               (b), the acquisition in torch and the selection by the search kernel.
Device ms between HIP events around --inner back-to-back calls after a warm-up of every call, median and min .. max over --reps rounds.
    python tools/gp_bench.py [--reps 7] [--inner 5] [--small] [--out profiles/gp_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.models.regression import GPHead, PropertyHead  # noqa: E402
from coati_amd.models.regression.gp_head import extractor_features  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gp_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, F, D, P, M = 256, 256, 4, 1, 60
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


torch.manual_seed(0)
head = PropertyHead(E, features=F, depth=D, num_outputs=P, unit_input=True)
gen = torch.Generator().manual_seed(1)
other = torch.nn.functional.normalize(torch.randn(M, E, generator=gen), dim=1).to(torch.bfloat16)
z = extractor_features(head, other)
l = 0.5 * float(torch.cdist(z, z).median())
q = (0.2 + 0.8 * torch.rand(M, M, generator=gen)) * 0.02 / M
gp = GPHead(head, z, torch.randn(P, M, generator=gen), q, None, l, 1.0, 0.05).to(dev)
head = gp.extractor

N = (1 << 20) // (64 if args.small else 1)
say(f"# python tools/gp_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, E={E} F={F} D={D} P={P} "
    f"M={M}, N={N}, device ms between HIP events per call, median (min .. max) over the rounds; (a) coati_head_eval, (b) coati_head_gp, "
    f"(c) coati_head_gp with the linear layer, (d) index.screen(gp, 10, acquisition='ucb')")
g = torch.Generator(device=dev).manual_seed(N)
index = EmbeddingIndex(E, metric="cosine", device=dev)
for lo in range(0, N, 1 << 18):
    index.add(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev))
x16 = index.vectors
fns = (lambda: head.predict_rows(x16), lambda: gp.gp_rows(x16), lambda: gp.gp_rows(x16, linear=True),
       lambda: index.screen(gp, 10, acquisition="ucb", beta=2.0))
for fn in fns:                                                # warm-up of every call the timed window uses
    fn()
    fn()
torch.cuda.synchronize()
t = [[] for _ in fns]
for _ in range(args.reps):
    for i, fn in enumerate(fns):
        t[i].append(timed(fn, args.inner))
a, b, c, d = (statistics.median(x) for x in t)
gb = x16.numel() * 2 / 1e9
mean, var, out = gp.gp_rows(x16, linear=True)
same = bool(torch.equal(out, head.predict_rows(x16)))
say(f"N={N:9d} ({gb:.3f} GB): (a) {spread(t[0])} ms = {gb / a * 1e3:7.1f} GB/s   (b) {spread(t[1])} ms   (c) {spread(t[2])} ms   "
    f"(d) {spread(t[3])} ms   (b)/(a) {b / a:6.3f}   (c)/(a) {c / a:6.3f}   (c)'s out == (a)'s: {same}   "
    f"var in {float(var.min()):.3g} .. {float(var.max()):.3g} of s2 = 1")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
