"""Prompt completion at the grande shape (d = 256, 16 layers, V = 10 322, n_seq = 250, random weights): Engine.generate_topk_batch
with prefill=True (decode_prefill over the shortest prompt's length, forced steps for the longer prompts' rest) against
prefill=False (every prompt token behind the first through a forced decode step), the two alternated in one process.

Per run: the time to the first sampled token of EVERY row (the sampler call at the longest prompt's end has completed), the whole
call, and generated tokens/s (sampled tokens that are not pads, over the whole call).  Two prompt sets: complete_batch-style prompts
of 10..40 tokens, and prompts of one length (40) where the prefill replaces every forced step.  Sampling: top-k 10 at inv_temp 2.

    python tools/generate_bench.py [--batch 1024] [--reps 3] [--json OUT]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from coati_amd import engine as E
    from coati_amd.engine import Engine, ModelConfig
    from oracle import coati_oracle as O
    kw = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16, n_seq=250,
              n_tok=10322)
    eng = Engine(ModelConfig(**kw), "cuda:0")
    eng.load_state_dict(O.init_params(O.OracleConfig(**kw), seed=1), strict=False)
    B = args.batch
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(10, 41, (B,), generator=g).tolist()
    ragged = [[2] + torch.randint(12, kw["n_tok"], (n - 1,), generator=g).tolist() for n in lens]
    uniform = [[2] + torch.randint(12, kw["n_tok"], (39,), generator=g).tolist() for _ in range(B)]

    # the time at which the sampler has drawn the first token of every row: the call at the longest prompt's end, synchronised
    real_call = E._lib.call
    mark = {}

    def call(name, *a):
        real_call(name, *a)
        if name == "coati_topk_sample_prompt" and a[10] == mark.get("pos") and "t" not in mark:
            torch.cuda.synchronize()
            mark["t"] = time.perf_counter()

    E._lib.call = call

    def run(prefix, prefill):
        mark.clear()
        mark["pos"] = max(len(p) for p in prefix)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.generate_topk_batch(prefix, stop_token=1, pad_token=0, inv_temp=2, k=10,
                                      generator=torch.Generator(device="cuda:0").manual_seed(1), prefill=prefill)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        gen = sum(sum(1 for t in row[len(p):] if t != 0) for row, p in zip(out, prefix))
        return {"ttft_ms": (mark["t"] - t0) * 1e3, "total_ms": (t1 - t0) * 1e3, "generated": gen, "tok_per_s": gen / (t1 - t0)}

    res = {}
    for name, prefix in (("ragged_10_40", ragged), ("uniform_40", uniform)):
        run(prefix, True)
        run(prefix, False)       # warm-up (workspace, kernel attributes)
        for rep in range(args.reps):
            for prefill in (True, False):
                r = run(prefix, prefill)
                res.setdefault(f"{name}/{'prefill' if prefill else 'steps'}", []).append(r)
                print(f"{name:14s} {'prefill' if prefill else 'steps  '} rep {rep}: first token of every row {r['ttft_ms']:8.2f} ms, "
                      f"call {r['total_ms']:8.1f} ms, {r['generated']} tokens, {r['tok_per_s']:9.0f} tok/s", flush=True)
    summary = {k: {m: sorted(x[m] for x in v)[len(v) // 2] for m in ("ttft_ms", "total_ms", "tok_per_s")} for k, v in res.items()}
    print(json.dumps({"batch": B, "median": summary}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"batch": B, "runs": res, "median": summary}, f, indent=1)


if __name__ == "__main__":
    main()
