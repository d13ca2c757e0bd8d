#!/usr/bin/env python3
"""Reads a rocprofv3 (rocpd sqlite) kernel trace.
  kern_seq.py results.db <name pattern> [N]    launch-ordered durations of the kernels matching a pattern, last N launches
  kern_seq.py --seq results.db [OUT.txt]       the whole launch sequence in dispatch order (the order the host enqueued them, whatever stream they
                                               ran on): one line (kernel name, grid, block) per launch into OUT.txt; prints the count and the
                                               SHA-256 of those lines as one JSON line -- two builds that launch the same kernels in the same
                                               order with the same geometry print the same hash"""
import hashlib
import json
import sqlite3
import sys


def sequence(db, out):
    c = sqlite3.connect(db)
    rows = c.execute("select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z from kernels order by dispatch_id").fetchall()
    text = ''.join(f'{r[0]} grid {r[1]}x{r[2]}x{r[3]} block {r[4]}x{r[5]}x{r[6]}\n' for r in rows)
    if out:
        with open(out, 'w') as f:
            f.write(text)
    print(json.dumps({'launches': len(rows), 'sha256': hashlib.sha256(text.encode()).hexdigest()}))


if sys.argv[1] == '--seq':
    sequence(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    sys.exit(0)
c = sqlite3.connect(sys.argv[1])
n = int(sys.argv[3]) if len(sys.argv) > 3 else 40
rows = c.execute("select name, grid_x/workgroup_x, duration from kernels where name like ? order by start desc limit ?",
                 ('%' + sys.argv[2] + '%', n)).fetchall()
for name, g, d in reversed(rows):
    print(f'{name[:60]:60s} grid {g:7d}  {d / 1e3:9.1f} us')
