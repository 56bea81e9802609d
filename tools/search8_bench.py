"""The quantised search (coati_search8_topk + coati_search_rescore through Fp8Index) against the bf16 search it approximates
(coati_search_topk, unchanged): per library (4 M rows x 256 and 1 M rows x 512, Gaussian), Q in {1, 16, 64, 1024} and k in {10, 100}, in one
process and alternated round by round, on prepared buffers,
  (a) coati_search_topk                                   the bf16 stream + the merge: the exact search;
  (b) coati_search8_topk at R = min(oversample * k, 128)  stage 1: the fp8 stream + the merge;
  (c) (b) + coati_search_rescore                          the two-stage search;   (c') Fp8Index.search(q, k): the same behind the host-side
      preparation and quantisation of the queries.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds.  Then recall@10 against the
exact search on a clustered library (1 M x 256, 4096 Gaussian centres + 0.5-sigma noise, cosine, 1024 queries of the same law): of the
two-stage result at oversample 1, 2, 4, 8, and of stage 1 alone.
python tools/search8_bench.py [--reps 5] [--inner 10] [--oversample 4] [--small] [--out profiles/search8_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd.fp8_index import R_MAX, quantise_device  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--oversample", type=int, default=4)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("search8_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
LIBS = [(4 << 20, 256), (1 << 20, 512)]
QS, KS = (1, 16, 64, 1024), (10, 100)
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


def filled(N, E, metric, draw):
    index = EmbeddingIndex(E, metric=metric, device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(draw(min(1 << 18, N - lo)))
    return index


say(f"# python tools/search8_bench.py --reps {args.reps} --inner {args.inner} --oversample {args.oversample}{' --small' if args.small else ''}: one MI355X, "
    "device ms between HIP events per call, median (min .. max) over the rounds; (a) coati_search_topk (bf16), (b) coati_search8_topk at R candidates "
    "(stage 1), (c) stage 1 + coati_search_rescore, (c') Fp8Index.search")
lib = _lib.lib()
for N, E in LIBS:
    N = N // 64 if args.small else N
    g = torch.Generator(device=dev).manual_seed(E)
    index = filled(N, E, "dot", lambda n: torch.randn(n, E, generator=g, device=dev))
    fp8 = index.fp8()
    lib16, lib8, scale = index.vectors, fp8.vectors8, fp8.scales
    say(f"## library {N} x {E}: bf16 {lib16.numel() * 2 / 1e9:.3f} GB, e4m3 + scales {(lib8.numel() + 4 * N) / 1e9:.3f} GB")
    for Q in QS:
        q = torch.randn(Q, E, generator=g, device=dev)
        q16 = q.to(torch.bfloat16)
        q8, qscale = quantise_device(q16)
        for k in KS:
            R = min(args.oversample * k, R_MAX)
            S, S8 = lib.coati_search_slices(N, Q, k), lib.coati_search8_slices(N, Q, R)
            need = Q * max(S * k, S8 * R)
            ps, pr = torch.empty(need, device=dev), torch.empty(need, dtype=torch.int32, device=dev)
            out_s, out_r = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.long, device=dev)
            c_s, c_r = torch.empty(Q, R, device=dev), torch.empty(Q, R, dtype=torch.long, device=dev)
            two_s, two_r = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.long, device=dev)

            def exact():
                _lib.call("coati_search_topk", ptr(lib16), N, E, ptr(index.bias), ptr(q16), Q, k, 1.0, S, ptr(ps), ptr(pr), ptr(out_s), ptr(out_r),
                          stream())

            def stage1():
                _lib.call("coati_search8_topk", ptr(lib8), ptr(scale), N, E, ptr(fp8.bias), ptr(q8), ptr(qscale), Q, R, 1.0, S8, ptr(ps), ptr(pr),
                          ptr(c_s), ptr(c_r), stream())

            def two():
                stage1()
                _lib.call("coati_search_rescore", ptr(lib16), N, E, ptr(index.bias), ptr(q16), Q, ptr(c_r), R, k, 1.0, ptr(two_s), ptr(two_r),
                          stream())

            fns = (exact, stage1, two, lambda: fp8.search(q, k, oversample=args.oversample))
            for fn in fns:                                    # warm-up of every shape the timed window uses
                fn()
            torch.cuda.synchronize()
            t = [[], [], [], []]
            for _ in range(args.reps):
                for i, fn in enumerate(fns):
                    t[i].append(timed(fn, args.inner))
            a, b, c, c2 = (statistics.median(x) for x in t)
            exact()
            two()
            torch.cuda.synchronize()
            hit = sum(len(set(x) & set(y)) for x, y in zip(out_r.tolist(), two_r.tolist())) / (Q * k)
            match = two_r[:, :, None] == out_r[:, None, :]                      # [Q, k, k]: where a returned row sits in the exact result
            bits = bool(((two_s == out_s.gather(1, match.float().argmax(dim=2))) | ~match.any(dim=2)).all())
            say(f"Q={Q:5d} k={k:3d} R={R:3d} S={S:3d}/{S8:3d}: (a) {spread(t[0])} ms   (b) {spread(t[1])} ms   (c) {spread(t[2])} ms   (b)/(a) {b / a:5.2f}   "
                f"(c)/(a) {c / a:5.2f}   (c') {c2:8.3f} ms   recall@{k} of (c) {100 * hit:.1f} %   shared rows' scores equal: {bits}")
    del index, fp8, lib16, lib8, scale
    torch.cuda.empty_cache()

# recall on a clustered library
N, E, Q, k, C = (1 << 20) // (64 if args.small else 1), 256, 1024, 10, 4096
g = torch.Generator(device=dev).manual_seed(7)
centres = torch.randn(C, E, generator=g, device=dev)


def draw(n):
    return centres[torch.randint(0, C, (n,), generator=g, device=dev)] + 0.5 * torch.randn(n, E, generator=g, device=dev)


index = filled(N, E, "cosine", draw)
fp8 = index.fp8()
q = draw(Q)
_, want = index.search(q, k)


def recall(rows):
    return 100 * sum(len(set(x) & set(y)) for x, y in zip(want.tolist(), rows.tolist())) / (Q * k)


say(f"## recall@{k} against the exact search: {N} x {E} cosine, {C} centres + 0.5-sigma noise, {Q} queries of the same law")
say(f"stage 1 alone (rescore=False): {recall(fp8.search(q, k, rescore=False)[1]):.2f} %")
for over in (1, 2, 4, 8):
    say(f"two stages, oversample={over} (R = {min(over * k, R_MAX)}): {recall(fp8.search(q, k, oversample=over)[1]):.2f} %")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
