"""Kernel table of a `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/score_grad_bench.py --routes ROUTE --reps 1 --iters N
--warmup W` run (ONE route): reads the rocpd SQLite output (NAME_results.db), takes the dispatches from the first call on (a packed call
starts with seq_len_kernel, a padded one with silu_fwd_kernel; what precedes is the weight set-up), counts the calls by their
ce_seq_bwd launches and prints every kernel's launches, time and share per call, the forward and the backward half apart (the
ce_seq_bwd launch ends the forward).    python tools/score_grad_profile.py DIR/NAME_results.db"""
import sqlite3
import sys
from collections import defaultdict


def table(title, rows, calls):
    agg = defaultdict(lambda: [0, 0.0])
    for name, t0, t1 in rows:
        a = agg[name.split("(")[0].split("<")[0][:60]]
        a[0] += 1
        a[1] += (t1 - t0) * 1e-3
    total = sum(v[1] for v in agg.values())
    print(f"== {title}: {len(rows)} dispatches in {calls} calls, kernel time {total / calls:.1f} us per call")
    print(f"{'kernel':62s} {'launches/call':>13s} {'us/call':>10s} {'share':>7s}")
    for name, (n, us) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{name:62s} {n / calls:13.1f} {us / calls:10.1f} {100 * us / total:6.1f}%")
    print()


def main(db):
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    seq = [i for i, r in enumerate(rows) if r[0].startswith("ce_seq_bwd_kernel")]
    assert seq, "no score_grad call in the trace"
    starts = ("seq_len_kernel", "silu_fwd_kernel")
    first = next(i for i, r in enumerate(rows) if r[0].startswith(starts))
    fwd, bwd, lo = [], [], first
    for k, s in enumerate(seq):
        fwd += rows[lo:s + 1]
        hi = seq[k + 1] if k + 1 < len(seq) else len(rows)
        # the next call's forward begins at its first seq_len / silu_fwd launch behind this call's ce_seq_bwd
        nxt = next((i for i in range(s + 1, hi) if rows[i][0].startswith(starts)), hi)
        bwd += rows[s + 1:nxt]
        lo = nxt
    table("score_grad, forward half (as coati_engine_score + lse / row factors)", fwd, len(seq))
    table("score_grad, backward half (dlogits, input gradients, [UNK] gather, token head)", bwd, len(seq))


if __name__ == "__main__":
    main(sys.argv[1])
