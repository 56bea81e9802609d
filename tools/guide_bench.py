"""The fused head-gradient kernel (coati_head_grad, csrc/guide.hip) against what torch offers for the same gradient and against its own
floor: E = F = 256, D = 4, P = 1 on bf16 Gaussian unit rows, N = 4096, 65536 and 1 M, in one process and alternated round by round,
  (a) coati_head_grad on prepared rows                      one launch: out [N, 1] and g [N, E] f32 written, nothing else;
  (b) PropertyHead.forward + torch.autograd.grad in f32     what there was before the kernel: 2 (D + 2) vendor GEMMs plus element-wise
      launches, every [N, F] activation written and read back;
  (c) the same chain with bf16 linears                       a bf16 copy of the head on the bf16 rows, autograd likewise;
  (d) coati_head_eval alone                                  the backward repeats the forward's flops: 2 (d) is the floor of this design;
  (e) one guided_ascent step                                 (a) plus prepare() and the update in torch, per step of an 8-step run.
Device ms between HIP events around `inner` back-to-back calls (more of them at small N, so that a window is not a fraction of a
millisecond), median and min .. max over --reps rounds; the ratios' spread is that of the per-round ratios.  TFLOP/s of (a) counts
2 * 2 N (E F + D F F + F P).   python tools/guide_bench.py [--reps 5] [--inner 5] [--small] [--out profiles/guide_bench.txt]"""
import argparse
import copy
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.generative import guided_ascent  # noqa: E402
from coati_amd.models.regression import PropertyHead  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("guide_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, F, D, P = 256, 256, 4, 1
STEPS = 8
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
    return f"{statistics.median(xs):8.4f} ({min(xs):.4f} .. {max(xs):.4f})"


def ratio(xs, ys, k=1.0):
    r = [x / (k * y) for x, y in zip(xs, ys)]
    return f"{statistics.median(r):6.3f} ({min(r):.3f} .. {max(r):.3f})"


torch.manual_seed(0)
head = PropertyHead(E, features=F, depth=D, num_outputs=P).to(dev)
head16 = copy.deepcopy(head).to(torch.bfloat16)


def torch_grad(model, x, cot):
    x = x.detach().requires_grad_(True)
    out = model(x)
    (g,) = torch.autograd.grad(out, x, cot.to(out.dtype))
    return out, g


say(f"# python tools/guide_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, E={E} F={F} D={D} P={P}, "
    f"device ms between HIP events per call, median (min .. max) over the rounds; (a) coati_head_grad, (b) forward + autograd.grad in f32, "
    f"(c) the same with bf16 linears, (d) coati_head_eval, (e) guided_ascent per step of {STEPS}")
for N in (4096, 65536, 1 << 20):
    N = max(64, N // 64) if args.small else N
    inner = max(args.inner, min(200, (1 << 22) // N))
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.nn.functional.normalize(torch.randn(N, E, generator=g, device=dev), dim=1)
    x16 = head.prepare(x)
    x32 = x16.float()
    cot = torch.randn(N, P, generator=g, device=dev)
    tflop = 2 * 2.0 * N * (E * F + D * F * F + F * P) / 1e12
    fns = (lambda: head.grad_rows(x16, cot), lambda: torch_grad(head, x32, cot), lambda: torch_grad(head16, x16, cot),
           lambda: head.predict_rows(x16), lambda: guided_ascent(x, head, steps=STEPS, lr=0.01))
    for fn in fns:                                            # warm-up of every shape the timed window uses
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[], [], [], [], []]
    for _ in range(args.reps):
        for i, fn in enumerate(fns):
            if i == 4:
                t[i].append(timed(fn, max(1, inner // STEPS)) / STEPS)
            else:
                t[i].append(timed(fn, inner))
    a = statistics.median(t[0])
    got, want = head.grad_rows(x16, cot)[1], torch_grad(head, x32, cot)[1]
    say(f"N={N:8d} (inner {inner:3d}): (a) {spread(t[0])} ms = {tflop / a * 1e3:6.1f} TFLOP/s   (b) {spread(t[1])} ms   (c) {spread(t[2])} ms   "
        f"(d) {spread(t[3])} ms   (e) {spread(t[4])} ms   (a)/(b) {ratio(t[0], t[1])}   (a)/(c) {ratio(t[0], t[2])}   "
        f"(a)/(2 (d)) {ratio(t[0], t[3], 2.0)}   max |(a) - (b)| / scale {float((got - want).abs().max()) / float(want.abs().max()):.2e}")
    del x, x16, x32, cot
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
