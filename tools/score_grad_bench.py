"""Cost of the likelihood gradient at the grande shape (random weights): Engine.score_grad (coati_engine_score_grad: the scoring forward,
per-row dlogits, the decoder pass's input gradients, the token head's backward) beside Engine.score on the same rows, B molecules of
T2 ~ 80 tokens, the caller's h_clip, on packed and on padded rows; as context the training step's forward(train=True) + backward()
(both passes, the point encoder, every weight gradient) on the same rows.
The routes are ALTERNATED in one process: `reps` rounds, each timing `iters` calls of every route between device events after a
synchronise; reported: the median over the rounds and their min .. max.
    python tools/score_grad_bench.py [--B 1024] [--T 82] [--iters 10] [--reps 5] [--warmup 2] [--routes a,b,...]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from coati_amd.engine import Engine, ModelConfig
from coati_amd.synthetic import make_batch

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
ROUTES = ("score_packed", "score_grad_packed", "score_padded", "score_grad_padded", "train_fwd_bwd_packed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=82)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default=",".join(ROUTES))
    args = ap.parse_args()
    routes = [r for r in args.routes.split(",") if r]
    assert all(r in ROUTES for r in routes) and args.reps >= 1, routes
    dev = torch.device("cuda:0")
    eng = Engine(ModelConfig(**GRANDE), dev, train="train_fwd_bwd_packed" in routes)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, (off, shape) in eng.layout.items():
            v = eng.view(name)
            if len(shape) == 2:
                v.copy_((torch.randn(shape, generator=g) * (0.02 if "tok_emb" not in name else 1.0)).to(dev))
            elif name.endswith("weight"):
                v.fill_(1.0)
    eng.refresh_shadows()
    B = args.B
    b, up = make_batch(B, args.T, 6, GRANDE["n_tok"], seed=1, min_len=12, p_bad=0.0, p_clip=1.0, with_rows=True)   # every row carries [CLIP][UNK]
    rows = b.pop("rows")
    b = {k: v.to(dev) for k, v in b.items()}
    up = up.to(dev)
    h = torch.randn(B, GRANDE["n_embd_common"], generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g)).to(dev)

    fns = {
        "score_packed": lambda: eng.score(b["tokens"], b["y_next"], h_clip=h, rows=rows),
        "score_grad_packed": lambda: eng.score_grad(b["tokens"], b["y_next"], h, weights=w, rows=rows),
        "score_padded": lambda: eng.score(b["tokens"], b["y_next"], h_clip=h),
        "score_grad_padded": lambda: eng.score_grad(b["tokens"], b["y_next"], h, weights=w),
        "train_fwd_bwd_packed": lambda: (eng.forward(b["raw_tokens"], b["tokens"], b["atoms"], b["coords"], up, y_next=b["y_next"], train=True,
                                                     rows=rows), eng.backward()),
    }
    for r in routes:
        for _ in range(args.warmup):
            fns[r]()
    torch.cuda.synchronize()
    ms = {r: [] for r in routes}
    for _ in range(args.reps):
        for r in routes:
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fns[r]()
            t1.record()
            torch.cuda.synchronize()
            ms[r].append(t0.elapsed_time(t1) / args.iters)
    out = {"B": B, "T2": int(b["tokens"].shape[1]), "rows": rows.tolist(), "iters": args.iters, "reps": args.reps}
    for r in routes:
        med = statistics.median(ms[r])
        out[r + "_ms"] = round(med, 3)
        out[r + "_ms_min_max"] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
        print(f"{r:22s}: median {med:8.3f} ms per call of {B} molecules (min {min(ms[r]):.3f} .. max {max(ms[r]):.3f} over {args.reps} rounds of {args.iters})",
              flush=True)
    for lay in ("packed", "padded"):
        if f"score_{lay}_ms" in out and f"score_grad_{lay}_ms" in out:
            out[f"score_grad_over_score_{lay}"] = round(out[f"score_grad_{lay}_ms"] / out[f"score_{lay}_ms"], 3)
    if "train_fwd_bwd_packed_ms" in out and "score_grad_packed_ms" in out:
        out["score_grad_over_train_fwd_bwd_packed"] = round(out["score_grad_packed_ms"] / out["train_fwd_bwd_packed_ms"], 3)
    if "score_grad_packed" in routes and "score_grad_padded" in routes:
        dk, dp = fns["score_grad_packed"]()[1].double(), fns["score_grad_padded"]()[1].double()
        out["dh_packed_vs_padded_worst_row"] = float(((dk - dp).abs().amax(1) / dp.abs().amax(1)).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
