"""Library density (include/coati_gmm.h): one EM iteration of a mixture of K diagonal Gaussians over a clustered bf16 library, per cell
  (a)  coati_gmm_estep alone, (b) coati_gmm_mstep alone (both launches), (c) the whole iteration of coati_amd.gmm.fit_rows' loop
       (parameter rows, both kernels, the float64 finish);
  (t)  the same iteration in torch on the same GPU: f32 matmul of [x | x^2] against par, logsumexp, two more matmuls -- its [N, K] and
       [N, 2E] temporaries and its peak memory included;
and once, sklearn.mixture.GaussianMixture(covariance_type="diag") on the host at 100 k rows.  For every kernel cell the fraction of the
f32 matrix peak (4 E K N flop per product pair / t against 155 TF) and of an HBM stream of the library (against 6.3 TB/s, the upper end of the measured streaming rates).
python tools/gmm_bench.py [--reps 5] [--inner 3] [--small] [--out profiles/gmm_bench.txt]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coati_amd import gmm as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--small", action="store_true", help="100 k and 1 M rows at K = 8 / 64 only")
ap.add_argument("--out", default="profiles/gmm_bench.txt")
args = ap.parse_args()
DEV = "cuda:0"
PEAK_F32, PEAK_HBM = 155e12, 6.3e12
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """the median over reps of the time of `inner` back-to-back calls, per call, in ms"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / args.inner)
    return sorted(out)[len(out) // 2]


def clustered(N, E, C=64, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cent = torch.randn(C, E, device=DEV, generator=g)
    out = torch.empty(N, E, dtype=torch.bfloat16, device=DEV)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        x = cent[torch.randint(0, C, (n,), device=DEV, generator=g)] + 0.5 * torch.randn(n, E, device=DEV, generator=g)
        out[lo:lo + n] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    return out


def start(x16, K):
    pick = torch.randperm(x16.shape[0], generator=torch.Generator().manual_seed(2))[:K].to(DEV)
    var = (x16[:100000].double().var(dim=0, unbiased=False) + 1e-6).expand(K, -1).clone()
    return torch.full((K,), 1.0 / K, dtype=torch.float64, device=DEV), x16[pick].double(), var


def torch_iteration(x16, par, cst):
    x = x16.float()
    xx = torch.cat([x, x * x], dim=1)
    logit = xx @ par.T + cst
    lse = torch.logsumexp(logit, dim=1)
    r = (logit - lse[:, None]).exp()
    return lse, r.sum(dim=0), r.T @ xx


say(f"# python tools/gmm_bench.py --reps {args.reps} --inner {args.inner}{' --small' if args.small else ''}: one MI355X, E = 256, clustered unit rows; ms per call")
E = 256
for N in ((100000, 1000000) if args.small else (1000000, 4000000)):
    x16 = clustered(N, E)
    for K in ((8, 64) if args.small else (8, 64, 256)):
        w, m, v = start(x16, K)
        par, cst = G.prepare_params(w, m, v, E)
        lse, _ = G.estep_call(x16, None, par, cst, want_assign=False)
        part = torch.empty(int(G._lib.lib().coati_gmm_part_floats(N, E, K)), dtype=torch.float32, device=DEV)
        te = timed(lambda: G.estep_call(x16, None, par, cst, want_assign=False))
        tm = timed(lambda: G.mstep_call(x16, None, par, cst, lse, part))

        def iteration():
            p, c = G.prepare_params(w, m, v, E)
            l, _ = G.estep_call(x16, None, p, c, want_assign=False)
            G._finish(*G.mstep_call(x16, None, p, c, l, part), w, m, v, N, 1e-6)

        ti = timed(iteration)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            tt = timed(lambda: torch_iteration(x16, par, cst))
            mem = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
            torch_s = f"{tt:9.3f} ms, {mem:6.2f} GiB of temporaries"
        except torch.cuda.OutOfMemoryError:
            torch_s = "out of memory"
        flop, stream = 4.0 * E * K * N, 2.0 * E * N
        say(f"N={N:8d} K={K:3d}: (a) estep {te:8.3f} ms = {flop / te / 1e9 / PEAK_F32 * 1e12 * 100:5.1f} % of the f32 matrix peak, {stream / te / 1e9 / PEAK_HBM * 1e12 * 100:5.1f} % of the "
            f"HBM stream   (b) mstep {tm:8.3f} ms = {2 * flop / tm / 1e9 / PEAK_F32 * 1e12 * 100:5.1f} % of the peak (its two product pairs)   (c) iteration {ti:8.3f} ms   (t) torch {torch_s}")
    del x16
try:
    from sklearn.mixture import GaussianMixture
    x16 = clustered(100000, E)
    xs = x16.double().cpu().numpy()
    for K in (8, 64):
        w, m, v = start(x16, K)
        sk = GaussianMixture(K, covariance_type="diag", tol=0, max_iter=5, reg_covar=1e-6, weights_init=w.cpu().numpy(), means_init=m.cpu().numpy(),
                             precisions_init=(1.0 / v).cpu().numpy())
        t0 = time.perf_counter()
        sk.fit(xs)
        say(f"sklearn on the host, 100000 x {E}, K={K}: {(time.perf_counter() - t0) / 5 * 1e3:9.1f} ms an iteration (5 iterations)")
except ImportError:
    say("sklearn is not installed: no host comparison")
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
