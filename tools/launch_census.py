#!/usr/bin/env python3
"""Launch census of a rocprofv3 --kernel-trace rocpd database: the multiset of (kernel name, grid, workgroup, LDS bytes) of the
whole run, for comparing two builds that must issue the same launches (a host-side refactor of the launchers).
    python tools/launch_census.py <a.db>             # count, geometry and name of every distinct launch
    python tools/launch_census.py <a.db> <b.db>      # the launches whose counts differ; exit status 1 if any do"""
import collections
import sqlite3
import sys


def census(path):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    geo = [k for k in cols if k.startswith(("grid", "workgroup", "lds"))]
    assert "name" in cols and geo, f"{path}: kernels view has columns {cols}"
    out = collections.Counter()
    for row in c.execute(f"select name, {', '.join(geo)} from kernels"):
        out[row] += 1
    return geo, out


def main():
    geo, a = census(sys.argv[1])
    print(f"# columns: name, {', '.join(geo)}")
    if len(sys.argv) < 3:
        for k, n in sorted(a.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"{n:7d}  {k[1:]}  {k[0][:120]}")
        return 0
    _, b = census(sys.argv[2])
    diff = sorted(k for k in set(a) | set(b) if a[k] != b[k])
    print(f"# launches {sum(a.values())} vs {sum(b.values())}, distinct (name, geometry) {len(a)} vs {len(b)}, differing {len(diff)}")
    for k in diff:
        print(f"{a[k]:7d} {b[k]:7d}  {k[1:]}  {k[0][:120]}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
