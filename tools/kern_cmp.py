#!/usr/bin/env python3
"""Same launches?  Compares (kernel name, grid, workgroup) of two rocprofv3 --kernel-trace runs (rocpd sqlite) of one program: as an
ordered sequence per stream where the `kernels` table has a stream column (streams matched by order of first launch), else as one ordered
sequence, and as a multiset.  The runtime's own copy kernels (__amd_rocclr_copyBuffer*: a hipMemcpy goes through them or through the DMA
engines, as the runtime sees fit at that moment -- torch's uploads of the inputs do) are left out of the sequences and counted apart.
Exit status 1 on any difference.  Usage: kern_cmp.py a_results.db b_results.db [dump prefix]"""
import collections
import sqlite3
import sys

RUNTIME_COPY = '__amd_rocclr_copyBuffer'


def launches(path):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute('pragma table_info(kernels)')]
    key = next((k for k in ('stream_id', 'stream', 'queue_id') if k in cols), None)
    dims = [d for d in ('grid_x', 'grid_y', 'grid_z', 'workgroup_x', 'workgroup_y', 'workgroup_z') if d in cols]
    rows = c.execute(f"select {key or '0'}, name, {', '.join(dims)} from kernels order by start").fetchall()
    seqs, copies = collections.OrderedDict(), collections.Counter()
    for r in rows:
        seqs.setdefault(r[0], [])
        if r[1].startswith(RUNTIME_COPY):
            copies[tuple(r[1:])] += 1
        else:
            seqs[r[0]].append(tuple(r[1:]))
    return key, list(seqs.values()), copies


(ka, a, ca), (kb, b, cb) = launches(sys.argv[1]), launches(sys.argv[2])
if len(sys.argv) > 3:
    for tag, q in (('a', a), ('b', b)):
        with open(f'{sys.argv[3]}_{tag}.txt', 'w') as f:
            for i, s in enumerate(q):
                f.writelines(f'{i}\t{t[0][:90]}\t{t[1:]}\n' for t in s)
print(f'split by: {ka or "nothing (one sequence)"}; streams {len(a)} / {len(b)}; launches {sum(map(len, a))} / {sum(map(len, b))}')
bad = ka != kb or len(a) != len(b)
for i, (x, y) in enumerate(zip(a, b)):
    if x != y:
        bad = True
        j = next((j for j, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
        print(f'stream {i}: {len(x)} / {len(y)} launches, first difference at {j}: {x[j] if j < len(x) else None} / {y[j] if j < len(y) else None}')
ma, mb = (collections.Counter(t for s in q for t in s) for q in (a, b))
print('multiset of launches:', 'equal' if ma == mb else f'differs: {list((ma - mb).items())[:5]} / {list((mb - ma).items())[:5]}')
print(f'runtime copy kernels (not compared): {sum(ca.values())} / {sum(cb.values())}', '' if ca == cb else f'-- {list((ca - cb).items())[:5]} / {list((cb - ca).items())[:5]}')
print('DIFFERENT' if bad or ma != mb else 'IDENTICAL')
sys.exit(1 if bad or ma != mb else 0)
