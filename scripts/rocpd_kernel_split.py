"""Kernel split of the last N forward passes in a rocprofv3 SQLite output (`rocprofv3 --kernel-trace --stats -d DIR -o NAME`
writes NAME_results.db): dispatches after the (N+1)-th-from-last dispatch of the marker kernel (the last kernel of one pass)
up to the last one, grouped by kernel name family. Prints a text table.

  python scripts/rocpd_kernel_split.py RESULTS.db --marker k_global_avg --passes 5
"""
import argparse
import re
import sqlite3
from collections import defaultdict


def family(name):
    n = name.replace("(anonymous namespace)::", "")
    n = re.sub(r"\(.*", "", n)
    n = re.sub(r"^void ", "", n)
    return n.replace("cd::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--marker", default="k_global_avg")
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    marks = [i for i, r in enumerate(rows) if a.marker in r[0]]
    assert len(marks) > a.passes, "fewer than %d passes in the trace" % (a.passes + 1)
    sel = rows[marks[-a.passes - 1] + 1:marks[-1] + 1]
    span_us = (sel[-1][2] - sel[0][1]) / 1e3
    tot = defaultdict(lambda: [0, 0.0])
    for name, s, e in sel:
        t = tot[family(name)]
        t[0] += 1
        t[1] += (e - s) / 1e3
    busy = sum(v[1] for v in tot.values())
    print("last %d passes: %d dispatches, %.1f us busy (%.1f us per pass), %.1f us wall span"
          % (a.passes, len(sel), busy, busy / a.passes, span_us))
    print("%-60s %8s %12s %7s" % ("kernel", "calls", "us/pass", "share"))
    for k, (n, us) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        print("%-60s %8d %12.1f %6.1f%%" % (k[:60], n // a.passes, us / a.passes, 100 * us / busy))


if __name__ == "__main__":
    main()
