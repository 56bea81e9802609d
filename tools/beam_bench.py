"""The beam-search step against the plain decode step at the grande shape (random weights): B = G * W = 1024 rows, W in {1, 4, 16}, 40
generated positions behind a 3-token prompt.  Per W: ms per beam step (coati_beam_row_topk + coati_beam_merge +
coati_engine_decode_step_beams) against ms per plain step (coati_engine_decode_step + coati_topk_sample, k = 1) at the same B, and the
share of the selection kernels; device time between HIP events, medians over the positions and over --reps repetitions, the two loops
alternated in one process.   python tools/beam_bench.py [--reps 3] [--out profiles/beam_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd.engine import Engine, ModelConfig  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
B, STEPS, PREFIX = 1024, 40, [8, 7, 2]
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
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
V, Tmax, m = eng.cfg.n_tok, eng.cfg.n_seq, len(PREFIX)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def prompt(payload):
    eng.decode_begin(B, Tmax)
    for i, t in enumerate(PREFIX):
        logits = eng.decode_step(torch.full((B,), t, dtype=torch.long, device=dev), payload if t == eng.cfg.unk_token else None,
                                 want_logits=(i == m - 1))
    return logits


def ev():
    return torch.cuda.Event(enable_timing=True)


def plain_loop(payload):
    """per position: ms of coati_topk_sample (k = 1), ms of decode_step"""
    logits = prompt(payload)
    u = torch.zeros(B, device=dev)
    marks = []
    for _ in range(STEPS):
        nxt = torch.empty(B, dtype=torch.long, device=dev)
        e = [ev(), ev(), ev()]
        e[0].record()
        _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, V, 1, 1.0, ptr(u), ptr(nxt), None, -1, 0, stream())
        e[1].record()
        logits = eng.decode_step(nxt)
        e[2].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [(e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])) for e in marks]


def beam_loop(payload, W):
    """per position: ms of row_topk + merge, ms of decode_step_beams (stop_token = -1: no hypothesis ever finishes)"""
    G = B // W
    logits = prompt(payload)
    cum = torch.full((G, W), float("-inf"), device=dev)
    cum[:, 0] = 0.0
    ident = torch.arange(B, dtype=torch.int32, device=dev).unsqueeze(1).repeat(1, Tmax).contiguous()
    cur = [cum.view(B), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), ident,
           torch.zeros(B, STEPS, dtype=torch.long, device=dev)]
    nxt = [torch.empty_like(cur[0]), torch.empty_like(cur[1]), torch.empty_like(cur[2]), ident.clone(), cur[4].clone()]
    cand_s, cand_t = torch.empty(B, W, device=dev), torch.empty(B, W, dtype=torch.int32, device=dev)
    tok_next, nfin = torch.empty(B, dtype=torch.long, device=dev), torch.zeros(G, dtype=torch.int32, device=dev)
    marks = []
    for n in range(STEPS):
        e = [ev(), ev(), ev()]
        e[0].record()
        _lib.call("coati_beam_row_topk", ptr(logits), logits.stride(0), G, W, V, ptr(cur[0]), ptr(cur[1]), 0, ptr(cand_s), ptr(cand_t), stream())
        _lib.call("coati_beam_merge", ptr(cand_s), ptr(cand_t), G, W, ptr(cur[0]), ptr(cur[1]), ptr(cur[2]), ptr(cur[3]), ptr(cur[4]), STEPS,
                  Tmax, m - 1 + n, n, -1, ptr(nxt[0]), ptr(nxt[1]), ptr(nxt[2]), ptr(nxt[3]), ptr(nxt[4]), ptr(tok_next), ptr(nfin), stream())
        cur, nxt = nxt, cur
        e[1].record()
        logits = eng.decode_step_beams(tok_next, cur[3])
        e[2].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [(e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])) for e in marks]


def med(rows, i):
    return statistics.median(r[i] for r in rows)


say(f"# python tools/beam_bench.py --reps {args.reps} (grande shape, random weights, B = G * W = {B}, {STEPS} generated positions {m} .. {m + STEPS - 1}), "
    "one MI355X; device ms between HIP events, median over the positions")
payload = torch.randn(B, eng.cfg.n_hidden_xformer, device=dev)
plain_loop(payload), beam_loop(payload, 4)          # warm-up
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    for W in (1, 4, 16):
        for rep in range(args.reps):
            p = plain_loop(payload)
            b = beam_loop(payload[::W].repeat_interleave(W, dim=0).contiguous(), W)
            ps, pd, bs, bd = med(p, 0), med(p, 1), med(b, 0), med(b, 1)
            say(f"W={W:2d} rep {rep}: plain step {ps + pd:.3f} ms (decode_step {pd:.3f} + topk_sample {ps:.3f}); beam step {bs + bd:.3f} ms "
                f"(decode_step_beams {bd:.3f} + row_topk and merge {bs:.3f} = {100 * bs / (bs + bd):.1f} %); beam / plain {(bs + bd) / (ps + pd):.3f}; "
                f"last position: decode_step {p[-1][1]:.3f}, decode_step_beams {b[-1][1]:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
