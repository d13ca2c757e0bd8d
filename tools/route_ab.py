#!/usr/bin/env python3
"""Fingerprint of the generator forward over every ACE route and chunk mode, for A/B runs of two builds of the library on one machine:
SHA-256 of the output bytes of each call and, from a second call of the same case with profiling on, launches / flops / flops_executed /
bytes of profile_read(kind) for kinds 0-3 (never ms).  Two builds that launch the same work on the same values write identical files.
Usage: route_ab.py <libctrlhair_hip.so> <out.json> [case name prefix]"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctrlhair_amd.lib as chlib  # noqa: E402

chlib.LIB_PATH = os.path.abspath(sys.argv[1])
from ctrlhair_amd import procedural as P  # noqa: E402
from ctrlhair_amd.sean.generator import SeanGenerator  # noqa: E402

NGF = 64
BIG = {'sean.ahead': 0}
# (name, f16x3 mode, options, max_batch, max_size, calls (B, S) in order on the one handle)
CASES = [
    ('default 1x128', 0, {}, 1, 128, [(1, 128), (1, 64), (1, 128)]),                 # full run-ahead, pad reuse
    ('ahead=0 3x128', 0, BIG, 3, 128, [(3, 128), (5, 128)]),                         # two chunks
    ('ahead=0 4x256', 0, BIG, 4, 256, [(4, 256), (3, 128)]),
    ('prologue=0 4x256', 0, dict(BIG, **{'sean.prologue': 0}), 4, 256, [(4, 256), (3, 128)]),
    ('lut_grouped=0 4x256', 0, dict(BIG, **{'sean.lut_grouped': 0}), 4, 256, [(4, 256), (3, 128)]),
    ('wino4_force=1 4x256', 0, dict(BIG, **{'sean.wino4_force': 1}), 4, 256, [(4, 256), (3, 128)]),
    ('batch_invariant=1 4x256', 0, dict(BIG, **{'sean.batch_invariant': 1}), 4, 256, [(4, 256), (3, 128)]),
    ('overlap=64 4x128', 0, dict(BIG, **{'sean.overlap': 64}), 4, 128, [(4, 128)]),
    ('wino=1 2x128', 0, {'sean.wino': 1}, 2, 128, [(2, 128)]),
    ('wino=1 gather=0 2x128', 0, {'sean.wino': 1, 'sean.wino_gather': 0}, 2, 128, [(2, 128)]),
    ('wino=0 2x128', 0, {'sean.wino': 0}, 2, 128, [(2, 128), (1, 128)]),             # B = 1: the tiny split-K levels
    ('sparse=0 2x128', 0, {'sean.sparse': 0}, 2, 128, [(2, 128)]),
    ('edge=0 2x128', 0, {'sean.edge': 0}, 2, 128, [(2, 128)]),
    ('patch=0 2x128', 0, {'sean.patch': 0}, 2, 128, [(2, 128)]),
]
for mode in (1, 2, 3):
    for dbg in (0, 64):
        CASES.append((f'f16x3={mode} dbg={dbg} 2x128', mode, {'sean.dbg': dbg} if dbg else {}, 2, 128, [(2, 128)]))


def inputs(kind, B, S):
    labels = P.blocky_labels(B, S, grid=8) if kind == 'blocky' else np.stack([P.face_like_labels(S, 40 + b) for b in range(B)])
    return [torch.from_numpy(a).cuda() for a in (labels, P.style_codes(B), P.noise_planes(B, S, NGF))]


def main():
    only = sys.argv[3] if len(sys.argv) > 3 else ''
    sd = P.sean_state_dict(0, NGF)
    result = {}
    for name, mode, opts, mb, ms, calls in CASES:
        if not name.startswith(only):
            continue
        gen = SeanGenerator(0, f16x3=mode, options=opts).load_state_dict(sd, max_batch=mb, max_size=ms)
        for i, (B, S) in enumerate(calls):
            for kind in ('blocky', 'face'):
                args = inputs(kind, B, S)
                out = gen.generate(*args)
                torch.cuda.synchronize()
                rec = {'sha256': hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}
                gen.handle.profile_enable(True)
                gen.generate(*args)
                torch.cuda.synchronize()
                gen.handle.profile_enable(False)
                for k in range(4):
                    r = gen.handle.profile_read(k)
                    rec[f'kind{k}'] = {f: r[f] for f in ('launches', 'flops', 'flops_executed', 'bytes')}
                gen.handle.profile_read(-1)
                result[f'{name} | call {i}: B={B} S={S} | {kind}'] = rec
                print(name, i, B, S, kind, rec['sha256'][:16], flush=True)
        gen.handle.close()
    with open(sys.argv[2], 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
