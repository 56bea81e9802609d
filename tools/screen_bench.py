"""The fused property-head kernel (coati_head_eval, csrc/screen.hip) against the layer-by-layer chain torch offers and against the memory
system: E = F = 256, D = 4, P = 1 on bf16 Gaussian unit rows, N = 1 M, 4 M (and 16 M with --big), in one process and alternated round by round,
  (a) coati_head_eval on the library's rows                 one launch, the library read once, [N, 1] floats written;
  (b) the torch bf16 chain on the same rows                  linear(x16, w0, b0), then h += relu(linear(h, w, b)) per block, then the last
      linear -- one vendor GEMM per layer over [N, F] bf16 activations, in chunks of --chunk rows so that the activations fit
      (its stream is rounded to bf16 after every layer, where (a)'s stays f32);
  (c) a device-to-device copy_ of the library's bytes        the bandwidth yardstick: it reads the library once (and writes it once);
  (d) index.screen(head, 10)                                 (a) plus the selection by the search kernel.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds; TFLOP/s = 2 N (E F + D F F + F P)
over the time.   python tools/screen_bench.py [--reps 5] [--inner 5] [--small] [--big] [--out profiles/screen_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.models.regression import PropertyHead  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--chunk", type=int, default=1 << 20)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--big", action="store_true", help="16 M rows as well")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("screen_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, F, D, P = 256, 256, 4, 1
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
head = PropertyHead(E, features=F, depth=D, num_outputs=P, unit_input=True).to(dev)
w0, b0 = head.first.weight.detach().to(torch.bfloat16), head.first.bias.detach().to(torch.bfloat16)
wr = [(r.weight.detach().to(torch.bfloat16), r.bias.detach().to(torch.bfloat16)) for r in head.residuals]
wl, bl = head.last.weight.detach().to(torch.bfloat16), head.last.bias.detach().to(torch.bfloat16)


def torch_chain(x16, out):
    for lo in range(0, x16.shape[0], args.chunk):
        h = torch.nn.functional.linear(x16[lo:lo + args.chunk], w0, b0)
        for w, b in wr:
            h += torch.relu_(torch.nn.functional.linear(h, w, b))
        out[lo:lo + args.chunk] = torch.nn.functional.linear(h, wl, bl)
    return out


say(f"# python tools/screen_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}{' --big' if args.big else ''}: one MI355X, "
    f"E={E} F={F} D={D} P={P}, device ms between HIP events per call, median (min .. max) over the rounds; (a) coati_head_eval, "
    f"(b) torch bf16 chain in chunks of {args.chunk} rows, (c) copy_ of the library, (d) index.screen(head, 10)")
for N in [1 << 20, 4 << 20] + ([16 << 20] if args.big else []):
    N = N // 64 if args.small else N
    g = torch.Generator(device=dev).manual_seed(N)
    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(torch.randn(min(1 << 18, N - lo), E, generator=g, device=dev))
    x16 = index.vectors
    dst = torch.empty_like(x16)
    out_b = torch.empty(N, P, dtype=torch.bfloat16, device=dev)
    gb, tflop = x16.numel() * 2 / 1e9, 2.0 * N * (E * F + D * F * F + F * P) / 1e12
    fns = (lambda: head.predict_rows(x16), lambda: torch_chain(x16, out_b), lambda: dst.copy_(x16), lambda: index.screen(head, 10))
    for fn in fns:                                            # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    t = [[], [], [], []]
    for _ in range(args.reps):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, args.inner))
    a, b, c, d = (statistics.median(x) for x in t)
    got, chain = head.predict_rows(x16)[:, 0], torch_chain(x16, out_b)[:, 0].float()
    scale = float(got.abs().max())
    say(f"N={N:9d} ({gb:.3f} GB): (a) {spread(t[0])} ms = {tflop / a * 1e3:6.1f} TFLOP/s, {gb / a * 1e3:7.1f} GB/s   (b) {spread(t[1])} ms = "
        f"{tflop / b * 1e3:6.1f} TFLOP/s   (c) {spread(t[2])} ms = {gb / c * 1e3:7.1f} GB/s   (d) {spread(t[3])} ms   (a)/(b) {a / b:6.3f}   "
        f"(a)/(c) {a / c:6.2f}   max |(a) - (b)| / scale {float((got - chain).abs().max()) / scale:.2e}")
    del index, x16, dst, out_b
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
