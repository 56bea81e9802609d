"""coati.generative throughput at the grande shape (d = 256, 16 heads, 16 layers, V = 10322, n_seq = 250), random weights:

1. embed_smiles_batch on synthetic SMILES of 38-76 tokens, B = 1024 per call: the reference's route (rows tokenized with pad=True, so
   T1 = 250, through encode_tokens) against the packed route (batch encode + coati_engine_encode_packed), molecules/s; host
   tokenization alone on its own line.
2. purify_vector looped over N vectors against purify_vectors, and force_decode_valid_batch looped against force_decode_valid_batches,
   vectors/s.  Random weights rarely draw [STOP], so the decodes run all n_seq - 3 steps: a full-length worst case.  The
   canonicaliser is the identity (every decode is valid: force_decode_valid_batch resolves on its first attempt).

The two routes of each item run alternately after a warm-up; device events bracket each call (the interval includes host work).

    python tools/generative_bench.py [--mols 10240] [--reps 3]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRANDE = dict(n_layer_e3gnn=5, n_layer_xformer=16, n_hidden_xformer=256, n_hidden_e3nn=256, n_embd_common=256, n_head=16,
              n_seq=250, n_tok=10322)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def tokenizer():
    from coati_amd.models.encoding.tokenizers import TrieTokenizer
    voc = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "tokenizer.json")))
    return TrieTokenizer(n_seq=250, special_tokens=voc["special"], smiles_tokens=[f"Z{i}Z" for i in range(GRANDE["n_tok"] - len(voc["special"]))])


def smiles(n, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(36, 75, (n,), generator=g).tolist()          # + [SMILES] + [STOP] = 38 .. 76 tokens
    ids = torch.randint(0, 10000, (n, 74), generator=g).tolist()
    return ["".join(f"Z{i}Z" for i in ids[k][:lens[k]]) for k in range(n)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=10240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="*", default=[8, 64])
    args = ap.parse_args()
    from coati.generative import coati_purifications as P
    from coati.common.util import batch_indexable
    from coati_amd.models.encoding.clip_e2e import e3gnn_smiles_clip_e2e
    with quiet():
        model = e3gnn_smiles_clip_e2e(**GRANDE, device=torch.device("cuda:0"))
    tk = tokenizer()
    print(f"grande: d = 256, 16 heads, 16 layers, V = 10322, n_seq = 250, random weights; {torch.cuda.get_device_name(0)}")

    # ---- 1. embed_smiles_batch -------------------------------------------------------------------------------------------------
    mols = smiles(args.mols, 1)
    t0 = time.perf_counter()
    for b in batch_indexable(mols, 1024):
        tk.encode_rows(["[SMILES]" + s + "[STOP]" for s in b])
    t_tok = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b in batch_indexable(mols, 1024):
        [tk.tokenize_text("[SMILES]" + s + "[STOP]", pad=True) for s in b]
    t_tok_ref = time.perf_counter() - t0

    def padded():
        outs = []
        for b in batch_indexable(mols, 1024):
            t = torch.tensor([tk.tokenize_text("[SMILES]" + s + "[STOP]", pad=True) for s in b], device="cuda:0", dtype=torch.int)
            outs.append(model.encode_tokens(t, tk))
        return torch.cat(outs)

    def packed():
        return torch.cat([P.embed_smiles_batch(b, model, tk) for b in batch_indexable(mols, 1024)])

    timed(padded), timed(packed)
    tp, tk_ = [], []
    for _ in range(args.reps):
        t, a = timed(padded)
        tp.append(t)
        t, b = timed(packed)
        tk_.append(t)
    err = float((a - b).abs().max())
    n = len(mols)
    print(f"embed_smiles_batch {n} molecules of 38-76 tokens, B = 1024 per call (ms per pass, best of {args.reps}; max |packed - padded| {err:.2e})")
    print(f"  padded route (tokenize_text pad=True, T1 = 250, encode_tokens) {min(tp):9.1f} ms  {n / min(tp) * 1e3:9.0f} molecules/s")
    print(f"  packed route (encode_rows, coati_engine_encode_packed)         {min(tk_):9.1f} ms  {n / min(tk_) * 1e3:9.0f} molecules/s")
    print(f"  host tokenization alone: encode_rows {t_tok * 1e3:.1f} ms, tokenize_text per row {t_tok_ref * 1e3:.1f} ms")

    # ---- 2. purification and forced decoding -------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    ident = lambda s: s  # noqa: E731
    with quiet():
        V8 = torch.randn(8, 256, device="cuda:0")
        P.purify_vectors(V8[:2], model, tk, n_rep=128, canon_smiles=ident, generator=gen)           # warm-up
        P.purify_vector(V8[0], model, tk, n_rep=128, canon_smiles=ident, generator=gen)
    for N in args.n:
        V = torch.randn(N, 256, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(N))
        with quiet():
            t_loop, _ = timed(lambda: [P.purify_vector(V[i], model, tk, n_rep=128, canon_smiles=ident, generator=gen) for i in range(N)])
            t_bat, out = timed(lambda: P.purify_vectors(V, model, tk, n_rep=128, canon_smiles=ident, generator=gen))
            f_loop, _ = timed(lambda: [P.force_decode_valid_batch(V[i], model, tk, canon_smiles=ident, generator=gen) for i in range(N)])
            f_bat, strs = timed(lambda: P.force_decode_valid_batches(V, model, tk, canon_smiles=ident, generator=gen))
        full = sum(len(tk.tokenize_text(s, pad=False, range_check=False)) >= 240 for s in strs)
        print(f"N = {N:3d} x n_rep 128 ({full}/{N} picked strings ran to >= 240 tokens: full-length worst case)")
        print(f"  purify_vector loop {t_loop:9.1f} ms {N / t_loop * 1e3:8.2f} vectors/s | purify_vectors {t_bat:9.1f} ms {N / t_bat * 1e3:8.2f} vectors/s "
              f"| x{t_loop / t_bat:.2f}")
        print(f"  force_decode_valid_batch loop {f_loop:9.1f} ms {N / f_loop * 1e3:8.2f} vectors/s | force_decode_valid_batches {f_bat:9.1f} ms "
              f"{N / f_bat * 1e3:8.2f} vectors/s | x{f_loop / f_bat:.2f}")


if __name__ == "__main__":
    main()
