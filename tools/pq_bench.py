"""The product-quantised search (coati_pq_topk + coati_search_rescore through PQIndex) against the exact bf16 search and the fp8 search:
per library (4 M and 1 M rows x 256, cosine, 4096 Gaussian centres + 0.5-sigma noise: search8_bench.py's clustered generator) and Q in
{1, 16, 64, 1024} at k = 10, in one process and alternated round by round,
  (a) EmbeddingIndex.search                 the exact search;
  (f) Fp8Index.search                       e4m3 rows, two stages at its default oversample;
  (p1) PQIndex.search(rescore=False)        stage 1 alone: the stream over the codes + the merge;
  (p2) PQIndex.search                       two stages at --oversample;
  (k) coati_pq_topk at R candidates         stage 1's two kernels on prepared buffers, without the host-side preparation.
Device ms between HIP events around --inner back-to-back calls, median and min .. max over --reps rounds.  Then the bytes held per row,
recall@10 against the exact search for stage 1 alone and for oversample 2 / 4 / 6 (1024 queries of the same law), the time to fit the
code books and the encoder's throughput.
python tools/pq_bench.py [--reps 5] [--inner 5] [--oversample 4] [--small] [--out profiles/pq_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib, pq as P  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402
from coati_amd.search import EmbeddingIndex, prepare_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--oversample", type=int, default=4)
ap.add_argument("--small", action="store_true", help="1/64 of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pq_bench: no GPU; nothing is measured without one")
dev = torch.device("cuda:0")
E, K, C = 256, 10, 4096
QS = (1, 16, 64, 1024)
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


say(f"# python tools/pq_bench.py --reps {args.reps} --inner {args.inner} --oversample {args.oversample}{' --small' if args.small else ''}: one MI355X, "
    "device ms between HIP events per call, median (min .. max) over the rounds; (a) EmbeddingIndex.search, (f) Fp8Index.search, (p1) PQIndex.search "
    "stage 1 alone, (p2) PQIndex.search two stages, (k) coati_pq_topk alone at R candidates")
lib = _lib.lib()
for N in (4 << 20, 1 << 20):
    N = N // 64 if args.small else N
    g = torch.Generator(device=dev).manual_seed(7)
    centres = torch.randn(C, E, generator=g, device=dev)

    def draw(n):
        return centres[torch.randint(0, C, (n,), generator=g, device=dev)] + 0.5 * torch.randn(n, E, generator=g, device=dev)

    index = EmbeddingIndex(E, metric="cosine", device=dev)
    for lo in range(0, N, 1 << 18):
        index.add(draw(min(1 << 18, N - lo)))
    fp8 = index.fp8()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    books = P.fit_codebooks(index.vectors)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    pq = index.pq(codebooks=books)
    enc = [timed(lambda: P.encode_device(index.vectors, books), 1) for _ in range(args.reps)]
    R = min(args.oversample * K, P.k_max(E))
    NP = 2 if E <= 128 else 1                       # pq.hip: query panels of a workgroup
    lds = 512 * E + 16 * NP * (R + 128) * 8 + 16 * NP * 8 + 8
    per_cu = min((160 << 10) // lds, 8)            # workgroups of 4 waves, one wave of each on every SIMD; 8 waves a SIMD at most
    say(f"## library {N} x {E} cosine, {C} centres + 0.5-sigma noise: bytes held per row: bf16 {2 * E + 4}, e4m3 {E + 8}, PQ {pq.bytes_per_row()} "
        f"(codes + bias; the two-stage searches hold the bf16 rows as well); code books {books.numel() * 2} bytes")
    say(f"fit_codebooks (65536 sampled rows, 20 rounds, torch): {t_fit:.2f} s; coati_pq_encode: {spread(enc)} ms = "
        f"{N / statistics.median(enc) * 1e3:.3e} rows/s")
    say(f"the scan at E = {E}, R = {R}: {lds} bytes of LDS a workgroup = {per_cu} workgroup(s) a CU = {per_cu} wave(s) a SIMD by LDS; "
        "VGPRs: see profiles/pq_resources.txt")
    q_all = draw(1024)
    for Q in QS:
        q = q_all[:Q].contiguous()
        _, q16 = prepare_queries(q, "cosine", E, dev)
        S = lib.coati_pq_slices(N, E, Q, R)
        ps, pr = torch.empty(Q * S * R, device=dev), torch.empty(Q * S * R, dtype=torch.int32, device=dev)
        c_s, c_r = torch.empty(Q, R, device=dev), torch.empty(Q, R, dtype=torch.long, device=dev)

        def kernel():
            _lib.call("coati_pq_topk", ptr(pq.codes), N, E, ptr(books), ptr(pq.bias), ptr(q16), Q, R, 1.0, S, ptr(ps), ptr(pr), ptr(c_s), ptr(c_r),
                      stream())

        fns = (lambda: index.search(q, K), lambda: fp8.search(q, K), lambda: pq.search(q, K, rescore=False),
               lambda: pq.search(q, K, oversample=args.oversample), kernel)
        for fn in fns:                                    # warm-up of every shape the timed window uses
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in fns]
        for _ in range(args.reps):
            for i, fn in enumerate(fns):
                t[i].append(timed(fn, args.inner))
        a, f, p1, p2, kk = (statistics.median(x) for x in t)
        say(f"Q={Q:5d} k={K} R={R} S={S:3d}: (a) {spread(t[0])} ms   (f) {spread(t[1])} ms   (p1) {spread(t[2])} ms   (p2) {spread(t[3])} ms   "
            f"(k) {spread(t[4])} ms   (p2)/(a) {p2 / a:5.2f}   (p2)/(f) {p2 / f:5.2f}   (k): {N * (E // 8 + 4) / kk / 1e6:.1f} GB/s of codes and bias")
    _, want = index.search(q_all, K)

    def recall(rows):
        return 100 * sum(len(set(x) & set(y)) for x, y in zip(want.tolist(), rows.tolist())) / (want.shape[0] * K)

    say(f"recall@{K} against the exact search, 1024 queries: stage 1 alone {recall(pq.search(q_all, K, rescore=False)[1]):.2f} %; " + "; ".join(
        f"oversample={o} (R = {min(o * K, P.k_max(E))}) {recall(pq.search(q_all, K, oversample=o)[1]):.2f} %" for o in (2, 4, 6)) +
        f"; Fp8Index {recall(fp8.search(q_all, K)[1]):.2f} %")
    del index, fp8, pq, books
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
