"""The fused acquisition-gradient kernel (coati_head_gp_grad, csrc/gp_grad.hip) against the two launches it joins and against what torch
offers for the same gradient: E = F = 256, D = 4, P = 1, M = 60 inducing points on bf16 Gaussian unit rows, N = 4096, 65536 and 1 M, in one
process and alternated round by round,
  (f) coati_head_gp_grad on prepared rows, ucb                one launch: mean [N, 1], var [N], acq [N] and g [N, E] f32 written, nothing else;
  (a) coati_head_gp, then coati_head_grad, back to back      the forward twice, the GP tail and the backward once each: the work the fused
      launch cannot undercut by much (it saves one forward and adds the GP's backward);
  (b) a torch bf16 chain with autograd                        bf16 linears and kernel matrix, mean + beta sqrt(var) in f32, autograd.grad
      with respect to the rows: vendor GEMMs plus element-wise launches, every [N, F] activation written and read back.
Device ms between HIP events around `inner` back-to-back calls (more of them at small N), median and min .. max over --reps rounds; the
ratios' spread is that of the per-round ratios.   python tools/acq_bench.py [--reps 5] [--inner 5] [--small] [--out profiles/acq_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd.models.regression import GPHead, PropertyHead  # noqa: E402
from coati_amd.models.regression.gp_head import extractor_features  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("acq_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, F, D, P, M = 256, 256, 4, 1, 60
BETA = 2.0
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


def ratio(xs, ys):
    r = [x / y for x, y in zip(xs, ys)]
    return f"{statistics.median(r):6.3f} ({min(r):.3f} .. {max(r):.3f})"


torch.manual_seed(0)
head = PropertyHead(E, features=F, depth=D, num_outputs=P)
gen = torch.Generator().manual_seed(1)
other = torch.nn.functional.normalize(torch.randn(M, E, generator=gen), dim=1).to(torch.bfloat16)
z = extractor_features(head, other)
l = 0.5 * float(torch.cdist(z, z).median())
q = (0.2 + 0.8 * torch.rand(M, M, generator=gen)) * 0.02 / M
gp = GPHead(head, z, torch.randn(P, M, generator=gen), q, None, l, 1.0, 0.05).to(dev)
head = gp.extractor
wm = torch.ones(P, device=dev)

# the torch chain's operands: the extractor's layers, z, alpha and the symmetric part of q in bf16 / f32 on the device
w16 = [head.first.weight.detach().to(torch.bfloat16)] + [r.weight.detach().to(torch.bfloat16) for r in head.residuals]
b16 = [head.first.bias.detach().to(torch.bfloat16)] + [r.bias.detach().to(torch.bfloat16) for r in head.residuals]
z16 = gp.z.to(torch.bfloat16)
zn = (gp.z.float() ** 2).sum(dim=1)
alpha32, c32 = (t.float() for t in gp._folded())
qs32 = (0.5 * (gp.q + gp.q.T)).float()
inv2l2, s2 = 1.0 / (2.0 * gp.lengthscale ** 2), gp.signal_var


def torch_chain(x16):
    x = x16.detach().requires_grad_(True)
    h = torch.nn.functional.linear(x, w16[0], b16[0])
    for w, b in zip(w16[1:], b16[1:]):
        h = h + torch.relu(torch.nn.functional.linear(h, w, b))
    d2 = ((h.float() ** 2).sum(dim=1)[:, None] + zn[None, :] - 2.0 * (h @ z16.T).float()).clamp_min(0.0)
    k = s2 * torch.exp(-d2 * inv2l2)
    mean = c32[None, :] + k @ alpha32.T
    var = (s2 - ((k @ qs32) * k).sum(dim=1)).clamp_min(0.0)
    acq = mean[:, 0] + BETA * var.sqrt()
    (g,) = torch.autograd.grad(acq.sum(), x)
    return acq, g


say(f"# python tools/acq_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, E={E} F={F} D={D} P={P} "
    f"M={M}, ucb with beta={BETA:g}, device ms between HIP events per call, median (min .. max) over the rounds; (f) coati_head_gp_grad, "
    f"(a) coati_head_gp + coati_head_grad back to back, (b) a torch bf16 chain with autograd")
for N in (4096, 65536, 1 << 20):
    N = max(64, N // 64) if args.small else N
    inner = max(args.inner, min(200, (1 << 22) // N))
    g = torch.Generator(device=dev).manual_seed(N)
    x16 = head.prepare(torch.nn.functional.normalize(torch.randn(N, E, generator=g, device=dev), dim=1))
    cot = torch.ones(N, P, device=dev)
    fns = (lambda: gp.acq_rows(x16, wm, BETA),
           lambda: (gp.gp_rows(x16), head.grad_rows(x16, cot)),
           lambda: torch_chain(x16))
    for fn in fns:                                            # warm-up of every shape the timed window uses
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.reps):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, inner))
    tflop = 2.0 * N * (2 * (E * F + D * F * F) + 2 * F * 64) / 1e12       # forward and backward of the layers, the z and zt products
    f = statistics.median(t[0])
    got, want = gp.acq_rows(x16, wm, BETA), torch_chain(x16)
    say(f"N={N:8d} (inner {inner:3d}): (f) {spread(t[0])} ms = {tflop / f * 1e3:6.1f} TFLOP/s   (a) {spread(t[1])} ms   (b) {spread(t[2])} ms   "
        f"(f)/(a) {ratio(t[0], t[1])}   (f)/(b) {ratio(t[0], t[2])}   max |g(f) - g(b)| / scale "
        f"{float((got[3] - want[1].float()).abs().max()) / float(want[1].float().abs().max()):.2e}   var in {float(got[1].min()):.3g} .. "
        f"{float(got[1].max()):.3g} of s2 = 1")
    del x16, cot
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
