"""Cost of COATI2 likelihood scoring and of its gradient at the full COATI2 shape (12 layers, d = 512, 16 heads of 32, V = 4266, seeded
random weights): Engine.score_coati2 and Engine.score_grad_coati2 on the same B rows of T2 <= 80 tokens under the caller's h_coati, on
packed and on padded rows.  The routes are ALTERNATED in one process: `reps` rounds, each timing `iters` calls of every route between
device events after a synchronise; reported: the median over the rounds and their min .. max.
    python tools/coati2_score_bench.py [--B 1024] [--T 80] [--iters 10] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from coati_amd.engine import Engine, ModelConfig

FULL = dict(n_layer_xformer=12, n_layer_e3gnn=0, n_hidden_xformer=512, n_hidden_e3nn=512, n_embd_common=512, n_head=16, n_seq=250, n_tok=4266,
            pad_token=31, stop_token=40, unk_token=44, use_point_encoder=False, enc_to_coati="swiglu_resnet")
ROUTES = ("score_coati2_packed", "score_grad_coati2_packed", "score_coati2_padded", "score_grad_coati2_padded")
CLIP, SMILES, N_SPECIAL = 2, 39, 330


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c = ModelConfig(**FULL)
    eng = Engine(c, dev, train=False)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, (off, shape) in eng.layout.items():
            v = eng.view(name)
            if len(shape) == 2:
                v.copy_((torch.randn(shape, generator=g) * (0.02 if "tok_emb" not in name else 1.0)).to(dev))
            elif name.endswith("weight"):
                v.fill_(1.0)
    eng.refresh_shadows()
    B, T = args.B, args.T
    n = torch.randint(12, T - 4 + 1, (B,), generator=g)          # body lengths: rows of 16 .. T tokens
    ar = torch.arange(T).unsqueeze(0)
    tok = torch.where((ar >= 3) & (ar < (3 + n).unsqueeze(1)), torch.randint(N_SPECIAL, c.n_tok, (B, T), generator=g),
                      torch.full((B, T), c.pad_token, dtype=torch.long))
    tok[:, 0], tok[:, 1], tok[:, 2] = CLIP, c.unk_token, SMILES
    tok[torch.arange(B), 3 + n] = c.stop_token
    y = torch.full_like(tok, -1)
    y[:, 2:-1] = tok[:, 3:]
    y[y == c.pad_token] = -1
    rows = (0, int((tok != c.pad_token).sum()))
    tok, y = tok.to(dev), y.to(dev)
    h = torch.randn(B, c.n_embd_common, generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g)).to(dev)
    fns = {
        "score_coati2_packed": lambda: eng.score_coati2(tok, y, h_coati=h, rows=rows),
        "score_grad_coati2_packed": lambda: eng.score_grad_coati2(tok, y, h, weights=w, rows=rows),
        "score_coati2_padded": lambda: eng.score_coati2(tok, y, h_coati=h),
        "score_grad_coati2_padded": lambda: eng.score_grad_coati2(tok, y, h, weights=w),
    }
    for r in ROUTES:
        for _ in range(args.warmup):
            fns[r]()
    torch.cuda.synchronize()
    ms = {r: [] for r in ROUTES}
    for _ in range(args.reps):
        for r in ROUTES:
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fns[r]()
            t1.record()
            torch.cuda.synchronize()
            ms[r].append(t0.elapsed_time(t1) / args.iters)
    out = {"B": B, "T2": T, "rows": list(rows), "iters": args.iters, "reps": args.reps}
    for r in ROUTES:
        med = statistics.median(ms[r])
        out[r + "_ms"] = round(med, 3)
        out[r + "_ms_min_max"] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
        print(f"{r:26s}: median {med:8.3f} ms per call of {B} molecules (min {min(ms[r]):.3f} .. max {max(ms[r]):.3f} over {args.reps} rounds of {args.iters})",
              flush=True)
    dk, dp = fns["score_grad_coati2_packed"]()[1].double(), fns["score_grad_coati2_padded"]()[1].double()
    out["dh_packed_vs_padded_worst_row"] = float(((dk - dp).abs().amax(1) / dp.abs().amax(1)).max())
    err = int(eng.scal[6:7].view(torch.int32).item())
    assert err == 0, err
    print(json.dumps(out))


if __name__ == "__main__":
    main()
