"""The syntax-constrained decode step against the plain one at the grande shape (random weights): B = 1024 rows, 40 generated positions
behind a 3-token prompt.  Per repetition: ms per plain step (coati_engine_decode_step + coati_topk_sample) against ms per constrained
step (the same two plus coati_grammar_step in front of the sampler), k = 100; device time between HIP events, medians over the positions,
the two loops alternated in one process.  Then one generate_top_k_with_inj_batch over all n_seq = 250 positions with and without the
grammar: the share of rows whose last position had to be overwritten with [STOP], and of rows that are not balanced.

The grammar is that of tests/golden/tokenizer_real.json (320 special + 2377 SMILES tokens of the real vocabulary), its SMILES entries
repeated cyclically up to the grande vocabulary size of 10 322: the table has the real entries' mix, the strings are those of the slice.
   python tools/grammar_bench.py [--reps 3] [--out profiles/grammar_bench.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from coati_amd import _lib  # noqa: E402
from coati_amd.engine import Engine, ModelConfig  # noqa: E402
from coati_amd.grammar import SmilesGrammar, balanced  # noqa: E402
from coati_amd.models.encoding.tokenizers import TrieTokenizer  # noqa: E402
from coati_amd.ops import ptr, stream  # noqa: E402

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)
B, STEPS, PREFIX, K, STOP = 1024, 40, [8, 7, 2], 100, 1
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

with open(os.path.join(ROOT, "tests", "golden", "tokenizer_real.json")) as f:
    fx = json.load(f)
tk = TrieTokenizer(n_seq=fx["n_seq"], smiles_tokens=fx["smiles"], special_tokens=fx["special"])
small = SmilesGrammar.from_tokenizer(tk)
n_special, n_smiles = len(fx["special"]), len(fx["smiles"])
cols = np.concatenate([np.arange(n_special), n_special + np.arange(V - n_special) % n_smiles])
gr = SmilesGrammar(small.need[:, cols], small.delta[:, cols], small.toggle[:, cols], small.flags[:, cols], STOP)
keys = [tk.keys[c] for c in cols]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def text(tokens):
    out = []
    for t in tokens:
        if t == STOP:
            break
        if t >= n_special:
            out.append(keys[t])
    return "".join(out)


def prompt(payload):
    eng.decode_begin(B, Tmax)
    for i, t in enumerate(PREFIX):
        logits = eng.decode_step(torch.full((B,), t, dtype=torch.long, device=dev), payload if t == eng.cfg.unk_token else None,
                                 want_logits=(i == m - 1))
    return logits


def ev():
    return torch.cuda.Event(enable_timing=True)


def loop(payload, grammar):
    """per position: ms of coati_grammar_step (0 without a grammar), of coati_topk_sample, of decode_step"""
    logits = prompt(payload)
    gen = torch.Generator(device=dev).manual_seed(1)
    state = grammar.states([grammar.walk(PREFIX, STEPS + m)] * B, dev) if grammar is not None else None
    prev, marks = None, []
    for n in range(STEPS):
        u = torch.rand(B, device=dev, generator=gen)
        nxt = torch.empty(B, dtype=torch.long, device=dev)
        e = [ev(), ev(), ev(), ev()]
        e[0].record()
        if grammar is not None:
            grammar.step(logits, state, state, tok_prev=prev, remaining=STEPS - n)
        e[1].record()
        _lib.call("coati_topk_sample", ptr(logits), logits.stride(0), B, V, K, 1.0, ptr(u), ptr(nxt), None, -1, 0, stream())
        e[2].record()
        logits = eng.decode_step(nxt)
        e[3].record()
        marks.append(e)
        prev = nxt
    torch.cuda.synchronize()
    return [(e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3])) for e in marks]


def med(rows, i):
    return statistics.median(r[i] for r in rows)


say(f"# python tools/grammar_bench.py --reps {args.reps} (grande shape, random weights, B = {B}, k = {K}, {STEPS} generated positions "
    f"{m} .. {m + STEPS - 1}), one MI355X; device ms between HIP events, median over the positions")
say(f"# expectation stated with the feature, not a pass mark: one more launch per step that reads about B x V x 12 B = "
    f"{B * V * 12 / 1e6:.0f} MB, mostly from cache, next to a plain step of 1.39 ms (k = 1; profiles/beam_bench.txt).  As built the launch "
    f"reads the B x V x 8 B = {B * V * 8 / 1e6:.0f} MB of table entries only: the mask does not depend on the logits")
payload = torch.randn(B, eng.cfg.n_hidden_xformer, device=dev)
loop(payload, None), loop(payload, gr)          # warm-up
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    for rep in range(args.reps):
        p, c = loop(payload, None), loop(payload, gr)
        ps, pd = med(p, 1), med(p, 2)
        cg, cs, cd = med(c, 0), med(c, 1), med(c, 2)
        say(f"rep {rep}: plain step {ps + pd:.3f} ms (decode_step {pd:.3f} + topk_sample {ps:.3f}); constrained step {cg + cs + cd:.3f} ms "
            f"(decode_step {cd:.3f} + topk_sample {cs:.3f} + grammar_step {cg:.3f} = {100 * cg / (cg + cs + cd):.1f} %); "
            f"constrained / plain {(cg + cs + cd) / (ps + pd):.3f}; grammar_step {B * V * 8 / cg / 1e6:.0f} GB/s of entries; "
            f"grammar_step first / last position {c[0][0]:.3f} / {c[-1][0]:.3f} ms")
for name, grammar in (("plain", None), ("grammar", gr)):
    rows = eng.generate_top_k_with_inj_batch(prefix=PREFIX, stop_token=STOP, pad_token=0, inv_temp=1.0, k=K, inj_token=eng.cfg.unk_token,
                                             inj_payload=payload, generator=torch.Generator(device=dev).manual_seed(2), grammar=grammar)
    over = int(eng.last_unstopped.sum())
    bad = sum(not balanced(text(r[m:])) for r in rows)
    viol = 0 if grammar is None else int(eng.last_grammar_violations.sum())
    say(f"generate_top_k_with_inj_batch, all {Tmax} positions, {name}: {over}/{B} rows had their last position overwritten with [STOP] "
        f"({100 * over / B:.1f} %), {bad}/{B} rows not balanced, {viol} rows flagged  (random weights hardly ever draw [STOP] by themselves)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
