"""Cost of a COATI2 training step (Engine.train_step on a COATI2 layout: encoder pass with the [STOP]-row tail, smiles_to_coati,
coati_to_token, decoder pass, lm_head CE, the whole backward with parameter gradients, clip-norm, AdamW) with seeded random weights, on B
rows of <= T tokens, packed rows: the full COATI2 shape (12 layers, d = 512, 16 heads of 32, V = 4266) and the d = 256 shape (16 layers, 16
heads of 16).  `reps` rounds of `iters` steps between device events after a synchronise; reported: the median over the rounds, min .. max.
    python tools/coati2_train_bench.py [--B 1024] [--T 80] [--iters 10] [--reps 5] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from coati_amd.engine import Engine, ModelConfig

COMMON = dict(n_layer_e3gnn=0, n_seq=250, n_tok=4266, pad_token=31, stop_token=40, unk_token=44, use_point_encoder=False, enc_to_coati="swiglu_resnet")
SHAPES = {"full_d512": dict(n_layer_xformer=12, n_hidden_xformer=512, n_hidden_e3nn=512, n_embd_common=512, n_head=16),
          "d256": dict(n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16)}
CLIP, SMILES, N_SPECIAL = 2, 39, 330


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T = args.B, args.T
    out = {"B": B, "T": T, "iters": args.iters, "reps": args.reps}
    for tag, shape in SHAPES.items():
        c = ModelConfig(**COMMON, **shape)
        eng = Engine(c, dev, train=True)
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for name, (off, shp) in eng.layout.items():
                v = eng.view(name)
                if len(shp) == 2:
                    v.copy_((torch.randn(shp, generator=g) * (0.02 if "tok_emb" not in name else 1.0)).to(dev))
                elif name.endswith("weight"):
                    v.fill_(1.0)
        eng.refresh_shadows()
        n = torch.randint(12, T - 4 + 1, (B,), generator=g)          # body lengths: decoder rows of 16 .. T tokens
        ar = torch.arange(T).unsqueeze(0)
        body = torch.randint(N_SPECIAL, c.n_tok, (B, T), generator=g)
        pad = torch.full((B, T), c.pad_token, dtype=torch.long)
        tok = torch.where((ar >= 3) & (ar < (3 + n).unsqueeze(1)), body, pad)
        tok[:, 0], tok[:, 1], tok[:, 2] = CLIP, c.unk_token, SMILES
        tok[torch.arange(B), 3 + n] = c.stop_token
        raw = torch.where((ar >= 1) & (ar < (1 + n).unsqueeze(1)), torch.roll(body, -2, 1), pad)      # [SMILES] + the same body + [STOP]
        raw[:, 0] = SMILES
        raw[torch.arange(B), 1 + n] = c.stop_token
        y = torch.full_like(tok, -1)
        y[:, 2:-1] = tok[:, 3:]
        y[y == c.pad_token] = -1
        rows = (int((raw != c.pad_token).sum()), int((tok != c.pad_token).sum()))
        batch = {"raw_tokens": raw.to(dev), "tokens": tok.to(dev), "y_next": y.to(dev), "rows": rows}
        for _ in range(args.warmup):
            eng.train_step(batch, None, 1e-4, do_clip=False)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                eng.train_step(batch, None, 1e-4, do_clip=False)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / args.iters)
        L = eng.losses()
        assert L["ar_loss"] == L["ar_loss"] and L["grad_norm"] > 0, L
        med = statistics.median(ms)
        out[tag] = {"ms_per_step": round(med, 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "rows": list(rows),
                    "ar_loss": round(L["ar_loss"], 4)}
        print(f"{tag:10s}: median {med:8.3f} ms per step of {B} molecules, packed rows {rows} (min {min(ms):.3f} .. max {max(ms):.3f} over "
              f"{args.reps} rounds of {args.iters}); ar loss {L['ar_loss']:.4f}", flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
