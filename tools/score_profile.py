"""Per-route kernel table of a `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/score_bench.py --iters N --warmup W` run:
reads the rocpd SQLite output (NAME_results.db) and splits the dispatches into the benchmark's three routes by the ce_seq launches
(each packed / padded call ends with one; the logits route has none), then prints, per route and call, every kernel's launches, time
and share.    python tools/score_profile.py DIR/NAME_results.db CALLS_PER_ROUTE"""
import sqlite3
import sys
from collections import defaultdict


def main(db, calls):
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    seq = [i for i, r in enumerate(rows) if r[0].startswith("ce_seq_kernel")]
    assert len(seq) == 2 * calls, (len(seq), calls)
    # a packed call starts with its seq_pack (seq_len_kernel) right behind the previous call's ce_seq; the first one with the first
    # seq_len_kernel of the run
    first = next(i for i, r in enumerate(rows) if r[0].startswith("seq_len_kernel"))
    bounds = {"packed": (first, seq[calls - 1] + 1), "padded": (seq[calls - 1] + 1, seq[2 * calls - 1] + 1),
              "logits": (seq[2 * calls - 1] + 1, len(rows))}
    for route, (lo, hi) in bounds.items():
        agg = defaultdict(lambda: [0, 0.0])
        for name, t0, t1 in rows[lo:hi]:
            a = agg[name.split("(")[0].split("<")[0][:60]]
            a[0] += 1
            a[1] += (t1 - t0) * 1e-3
        total = sum(v[1] for v in agg.values())
        print(f"== {route}: {hi - lo} dispatches in {calls} calls, kernel time {total / calls:.1f} us per call")
        print(f"{'kernel':62s} {'launches/call':>13s} {'us/call':>10s} {'share':>7s}")
        for name, (n, us) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"{name:62s} {n / calls:13.1f} {us / calls:10.1f} {100 * us / total:6.1f}%")
        print()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
