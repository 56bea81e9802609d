"""Streamed generation against chunked aligned generation at the grande shape (d = 256, 16 layers, V = 10 322, n_seq = 250, random
weights), one process, the routes alternated, medians of --reps runs.

Random weights never draw [STOP], so the row lengths are FORCED: request n carries a full row of len[n] tokens ending in [STOP], which
both routes emit through their sampler's prompt rule (no draw; every step still runs the whole transformer step and the sampler
launch).  len comes from a seeded distribution written into the record:
    uniform     38 .. 76 tokens (the lengths of profiles/generative_bench.txt)
    long_tail   30 + floor(Exp(mean 25)), capped at n_seq: most rows short, a few several times the mean
Routes, for N = 10 240 requests with an injection row each:
    (a) chunks of B = 1024 through the aligned loop (decode_begin, decode_step for every position, coati_topk_sample_prompt, one
        host look at `stopped` per step): what generate_topk_batch(prefill=False) runs; a chunk takes max(len) - 1 steps
    (b) Engine.generate_stream on 1024 slots (poll = 1 and poll = 4)
Printed per route: molecules/s, tokens/s, steps; and the ceiling the lengths allow: sum over chunks of (max len - 1) steps against
ceil(sum (len - 1) / B), with the fraction of it the stream reached.

Second part: the complete_batch case of tools/generate_bench.py (prompts of 10 .. 40 tokens, B = 1024, top-k 10 at inv_temp 2) with
ragged=True next to prefill=True and prefill=False: time to the first sampled token of every row, and the whole call.

    python tools/stream_bench.py [--n 10240] [--batch 1024] [--reps 3] [--skip-stream | --skip-complete] [--json OUT]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def lengths(name, N, n_seq, seed):
    g = torch.Generator().manual_seed(seed)
    if name == "uniform":
        return torch.randint(38, 77, (N,), generator=g)
    e = -25.0 * torch.log(1.0 - torch.rand(N, generator=g))
    return (30 + e.floor().to(torch.int64)).clamp(max=n_seq)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10240)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-complete", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    args = ap.parse_args()
    from coati_amd import engine as E
    from coati_amd.engine import Engine, ModelConfig
    from coati_amd.ops import ptr, stream
    from oracle import coati_oracle as O
    kw = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16, n_seq=250,
              n_tok=10322)
    eng = Engine(ModelConfig(**kw), DEV)
    eng.load_state_dict(O.init_params(O.OracleConfig(**kw), seed=1), strict=False)
    c = eng.cfg
    N, B, n_seq, stop, pad, k, inv_temp = args.n, args.batch, c.n_seq, c.stop_token, c.pad_token, 10, 2.0
    record = {"n": N, "batch": B, "reps": args.reps, "k": k, "inv_temp": inv_temp}

    def aligned_chunk(prompt_d, plen_d, longest, inj):
        """the loop of Engine._complete_on_stream with prefill=False on one chunk; returns (tokens [b, longest], steps)"""
        b = prompt_d.shape[0]
        out = torch.zeros(b, n_seq, dtype=torch.long, device=DEV)
        out[:, 0] = prompt_d[:, 0]
        stopped = (prompt_d[:, :1] == stop).any(1).to(torch.int32)
        eng.decode_begin(b, n_seq)
        logits = eng.decode_step(out[:, 0], inj)
        pos, steps = 1, 1
        while pos < n_seq:
            u = torch.rand(b, device=DEV)
            nxt = torch.empty(b, dtype=torch.long, device=DEV)
            E._lib.call("coati_topk_sample_prompt", ptr(logits), logits.stride(0), b, c.n_tok, k, inv_temp, ptr(u), ptr(prompt_d),
                        prompt_d.stride(0), ptr(plen_d), pos, ptr(nxt), ptr(stopped), stop, pad, stream())
            out[:, pos] = nxt
            pos += 1
            if pos >= n_seq or (pos >= longest and int(stopped.sum().item()) >= b):
                break
            logits = eng.decode_step(nxt, inj)
            steps += 1
        return out[:, :pos], steps

    for dist in () if args.skip_stream else ("uniform", "long_tail"):
        lens = lengths(dist, N, n_seq, seed=7)
        g = torch.Generator().manual_seed(8)
        W = int(lens.max())
        forced = torch.randint(12, c.n_tok, (N, W), generator=g)
        forced[:, 0], forced[:, 1], forced[:, 2] = 8, c.unk_token, 2
        forced[torch.arange(N), lens - 1] = stop
        payload = torch.randn(N, c.n_hidden_xformer, generator=g).to(DEV)
        forced_d, lens_d = forced.to(DEV), lens.to(torch.int32).to(DEV)
        chunks = [(lo, min(N, lo + B)) for lo in range(0, N, B)]
        ceil_a = sum(int(lens[lo:hi].max()) - 1 for lo, hi in chunks)
        ceil_b = math.ceil(int((lens - 1).sum()) / B)
        n_tok = int(lens.sum())

        def route_a():
            side = torch.cuda.Stream(device=DEV)
            rows, steps = [], 0
            with torch.cuda.stream(side):
                for lo, hi in chunks:
                    r, s = aligned_chunk(forced_d[lo:hi], lens_d[lo:hi], int(lens[lo:hi].max()), payload[lo:hi])
                    rows.append(r.cpu())
                    steps += s
            return rows, steps

        def route_b(poll):
            rows = eng.generate_stream([8], stop, pad, inv_temp, k, c.unk_token, payload, slots=B, as_tensor=True, poll=poll,
                                       generator=torch.Generator(device=DEV).manual_seed(1), forced=(forced_d, lens_d)).cpu()
            return rows, eng.stream_steps

        routes = {"a_chunked": route_a, "b_stream_poll1": lambda: route_b(1), "b_stream_poll4": lambda: route_b(4)}
        for fn in routes.values():     # warm-up (workspaces, kernel attributes) and a check: both routes return the forced rows
            rows, _ = fn()
            if isinstance(rows, list):
                for (lo, hi), r in zip(chunks, rows):
                    for n in range(lo, hi, 97):
                        assert r[n - lo, : lens[n]].tolist() == forced[n, : lens[n]].tolist()
            else:
                for n in range(0, N, 97):
                    assert rows[n, : lens[n]].tolist() == forced[n, : lens[n]].tolist()
        times = {name: [] for name in routes}
        steps = {}
        for rep in range(args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, steps[name] = fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                print(f"{dist:9s} {name:15s} rep {rep}: {times[name][-1] * 1e3:8.1f} ms, {steps[name]} steps", flush=True)
        out = {"lengths": {"min": int(lens.min()), "max": int(lens.max()), "mean": float(lens.float().mean()), "tokens": n_tok},
               "ceiling_steps": {"chunked": ceil_a, "ideal": ceil_b}}
        for name in routes:
            t = median(times[name])
            out[name] = {"ms": t * 1e3, "ms_min": min(times[name]) * 1e3, "ms_max": max(times[name]) * 1e3, "steps": steps[name],
                         "molecules_per_s": N / t, "tokens_per_s": n_tok / t, "ms_per_step": t * 1e3 / steps[name]}
        spread_a = (max(times["a_chunked"]) - min(times["a_chunked"])) / median(times["a_chunked"])
        out["spread_a"] = spread_a
        out["speedup_poll1"] = median(times["a_chunked"]) / median(times["b_stream_poll1"])
        out["speedup_poll4"] = median(times["a_chunked"]) / median(times["b_stream_poll4"])
        out["fraction_of_ceiling_poll1"] = ceil_b / steps["b_stream_poll1"]
        out["fraction_of_ceiling_poll4"] = ceil_b / steps["b_stream_poll4"]
        record[dist] = out
        print(f"{dist}: lengths {out['lengths']}, ceiling {ceil_a} -> {ceil_b} steps ({ceil_a / ceil_b:.2f}x)")
        for name in routes:
            o = out[name]
            print(f"  {name:15s} {o['ms']:8.1f} ms ({o['ms_min']:.1f} .. {o['ms_max']:.1f}), {o['steps']:5d} steps, {o['ms_per_step']:.3f} ms/step, "
                  f"{o['molecules_per_s']:8.0f} molecules/s, {o['tokens_per_s']:9.0f} tokens/s")
        print(f"  stream / chunked: {out['speedup_poll1']:.3f}x (poll 1), {out['speedup_poll4']:.3f}x (poll 4); run-to-run spread of the "
              f"chunked route {spread_a * 100:.1f} %; fraction of the length ceiling reached {out['fraction_of_ceiling_poll1']:.3f} / "
              f"{out['fraction_of_ceiling_poll4']:.3f}", flush=True)

    if not args.skip_complete:
        g = torch.Generator().manual_seed(0)
        plens = torch.randint(10, 41, (B,), generator=g).tolist()
        prompts = [[2] + torch.randint(12, c.n_tok, (n - 1,), generator=g).tolist() for n in plens]
        real_call = E._lib.call
        mark = {}

        def call(name, *a):
            real_call(name, *a)
            first = (name == "coati_topk_sample_prompt" and a[10] == mark.get("pos")) or name == "coati_topk_sample_rows"
            if first and "t" not in mark:      # the sampler call after which every row has its first sampled token
                torch.cuda.synchronize()
                mark["t"] = time.perf_counter()

        E._lib.call = call

        def run(mode):
            mark.clear()
            mark["pos"] = max(plens)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.generate_topk_batch(prompts, stop_token=stop, pad_token=pad, inv_temp=2, k=10, generator=torch.Generator(device=DEV).manual_seed(1),
                                    prefill=(mode != "steps"), ragged=(mode == "ragged"))
            torch.cuda.synchronize()
            return {"ttft_ms": (mark["t"] - t0) * 1e3, "total_ms": (time.perf_counter() - t0) * 1e3}

        modes = ("prefill", "steps", "ragged")
        for _ in range(2):      # warm-up: workspaces, kernel attributes, the allocator's blocks of this part's sizes
            for m in modes:
                run(m)
        res = {m: [] for m in modes}
        for rep in range(args.reps):
            for m in modes:
                res[m].append(run(m))
                print(f"complete 10..40 {m:8s} rep {rep}: first token of every row {res[m][-1]['ttft_ms']:8.2f} ms, call {res[m][-1]['total_ms']:8.1f} ms",
                      flush=True)
        E._lib.call = real_call
        record["complete_10_40"] = {m: {"ttft_ms": median([r["ttft_ms"] for r in v]), "ttft_ms_min": min(r["ttft_ms"] for r in v),
                                        "ttft_ms_max": max(r["ttft_ms"] for r in v), "total_ms": median([r["total_ms"] for r in v])}
                                    for m, v in res.items()}
    print(json.dumps(record))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
