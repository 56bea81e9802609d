"""Likelihood-scoring throughput at the grande shape (random weights): molecules/s of the round-trip (s2s) NLL of B molecules of
T ~ 80 tokens on three routes --
  packed : Engine.score(raw_tokens=...) on packed rows (coati_engine_score: encoder pass, special token, decoder pass, lm_head CE
           partials, ce_seq)
  padded : the same call on the padded [B, T] layout
  logits : the route without it: Engine.forward(use_point = 0) + Engine.logits() (f32 [B*T, V]) + torch cross-entropy per row
Each route: warm-up, then a synchronised window of device events around `iters` calls.
    python tools/score_bench.py [--B 1024] [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from coati_amd.engine import Engine, ModelConfig
from coati_amd.synthetic import make_batch

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=82)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = Engine(ModelConfig(**GRANDE), dev, train=False)
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
    b, _ = make_batch(B, args.T, 6, GRANDE["n_tok"], seed=1, min_len=12, p_bad=0.0, with_rows=True)
    rows = b.pop("rows")
    b = {k: v.to(dev) for k, v in b.items()}
    no_point = torch.zeros(B, dtype=torch.uint8, device=dev)

    def packed():
        return eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"], rows=rows)

    def padded():
        return eng.score(b["tokens"], b["y_next"], raw_tokens=b["raw_tokens"])

    def logits_route():
        eng.forward(b["raw_tokens"], b["tokens"], b["atoms"], b["coords"], no_point, y_next=b["y_next"], train=False)
        lg = eng.logits()
        ce = torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), b["y_next"].reshape(-1), ignore_index=-1, reduction="none")
        return ce.view(B, -1).sum(1)

    out = {"B": B, "T2": int(b["tokens"].shape[1]), "rows": rows.tolist(), "iters": args.iters}
    results = {}
    for name, fn in (("packed", packed), ("padded", padded), ("logits", logits_route)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            r = fn()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.iters
        results[name] = r.double().cpu()
        out[f"{name}_ms"] = round(ms, 3)
        out[f"{name}_mol_per_s"] = round(B / (ms * 1e-3), 1)
        print(f"{name:7s}: {ms:8.3f} ms per call of {B} molecules = {B / (ms * 1e-3):10.0f} molecules/s", flush=True)
    for name in ("padded", "logits"):
        d = (results["packed"] - results[name]).abs() / results[name].abs().clamp(min=1e-30)
        out[f"packed_vs_{name}_max_rel"] = float(d.max())
    out["speedup_packed_vs_logits"] = round(out["logits_ms"] / out["packed_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
