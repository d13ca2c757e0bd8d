"""SHA-256 of the generator's output over the ACE-side list of calls, and the profile records of kinds 0-3 of one call per handle, as JSON.

    python tools/level_plan_digest.py OUT.json

The sibling of conv_route_digest.py (whose put() it reuses) for the host schedule of the ACEs: two builds that classify every level alike,
take every ACE down the same route and hand every launch the same operands give the same file.  The handles reach every branch of the
per-chunk plan (sean_model.cpp Runner::plan_aces / prepare): full run-ahead, prologue with per-ACE and with grouped LUTs, inline ACE
products, prepass + overlap, each of the switches that change a level's marks or lists, the direct sparse route with two tile shapes on one
level, a level max_size does not have, and the f16 paths in their three compaction modes.  ngf = 16; every entry is computed twice.
Profiling switches the side stream and the prologue off, so the records fingerprint the inline schedule only.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_route_digest as D                            # noqa: E402
from ctrlhair_amd import procedural as P                 # noqa: E402
from ctrlhair_amd.sean.generator import SeanGenerator    # noqa: E402

NGF = D.NGF
AHEAD0 = {'sean.ahead': 0}
F32_DEFAULT_CALLS = [(B, S) for S in (64, 128, 256) for B in (1, 3)]      # conv_route_digest.py's f32 list
SWITCHES = ('sean.wino_gather', 'sean.edge', 'sean.frame', 'sean.patch', 'sean.hidden_wq', 'sean.sparse', 'sean.wino')
# (tag, path, options, max_batch, max_size, calls (B, S))
HANDLES = [('f32', 'f32', {}, 2, 256, F32_DEFAULT_CALLS),
           ('f32_mb3', 'f32', AHEAD0, 3, 256, [(3, 256), (3, 128), (5, 128)]),
           ('f32_mb4', 'f32', AHEAD0, 4, 256, [(4, 256), (4, 128), (3, 128)]),
           ('f32_mb4_prologue0', 'f32', dict(AHEAD0, **{'sean.prologue': 0}), 4, 256, [(4, 256), (4, 128), (3, 128)]),
           ('f32_mb4_overlap64', 'f32', dict(AHEAD0, **{'sean.overlap': 64}), 4, 256, [(4, 256)])]
HANDLES += [(f'f32_mb3_{k.split(".")[1]}0', 'f32', dict(AHEAD0, **{k: 0}), 3, 256, [(3, 256)]) for k in SWITCHES]
HANDLES += [('f32_ms96', 'f32', {}, 2, 96, [(2, 64)])]
HANDLES += [(f'{path}_compact{c}', path, {'sean.sh16_compact': c}, 2, 256, [(3, 128), (3, 256)])
            for path in ('f16x3', 'f16', 'bf16') for c in (0, 1, 2)]
records = {}


def inputs(B, S, dev):
    return (torch.from_numpy(P.blocky_labels(B, S, grid=8, seed=100 + S)).to(dev), torch.from_numpy(P.style_codes(B, seed=200 + S)).to(dev),
            torch.from_numpy(P.noise_planes(B, S, NGF, seed=300 + S)).to(dev))


def handle_calls(sd, tag, path, options, mb, ms, calls):
    g = SeanGenerator(0, f16x3=D.PATHS[path], options=options).load_state_dict(sd, max_batch=mb, max_size=ms)
    for B, S in calls:
        lab, codes, noise = inputs(B, S, g.device)

        def run():
            out = g.generate(lab, codes, noise)
            torch.cuda.synchronize()
            return {'image': out.cpu().numpy()}
        D.put(f'gen/{tag}/S{S}_B{B}', run)
    B, S = calls[0]
    lab, codes, noise = inputs(B, S, g.device)
    g.handle.profile_enable(True)
    g.generate(lab, codes, noise)
    torch.cuda.synchronize()
    rec = {}
    for kind in (0, 1, 2, 3):
        r = g.handle.profile_read(kind)
        rec[f'kind{kind}'] = {k: r[k] for k in ('launches', 'flops', 'flops_executed', 'bytes')}
    g.handle.profile_read(-1)
    g.handle.profile_enable(False)
    records[f'gen/{tag}/S{S}_B{B}'] = rec
    g.handle.close()


TRACED = ('f32', 'f32_mb3', 'f32_mb4', 'f32_mb4_prologue0', 'f32_mb4_overlap64', 'f32_mb3_wino0', 'f32_ms96', 'f16x3_compact1')


def trace_calls(sd):
    """the fixed subset for a kernel trace (rocprofv3 --kernel-trace -- python tools/level_plan_digest.py --trace; tools/kern_seq.py --seq
    reads it): every call of these handles, once"""
    for tag, path, options, mb, ms, calls in HANDLES:
        if tag not in TRACED:
            continue
        g = SeanGenerator(0, f16x3=D.PATHS[path], options=options).load_state_dict(sd, max_batch=mb, max_size=ms)
        for B, S in calls:
            g.generate(*inputs(B, S, g.device))
            torch.cuda.synchronize()
        g.handle.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else 'level_plan_digest.json'
    sd = P.sean_state_dict(0, NGF)
    if out == '--trace':
        return trace_calls(sd)
    for h in HANDLES:
        handle_calls(sd, *h)
    res = {'digests': D.digests, 'unstable_max_abs_diff': D.unstable, 'profile_kinds': records}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'entries': len(D.digests), 'unstable': D.unstable}))


if __name__ == '__main__':
    main()
