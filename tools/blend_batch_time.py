#!/usr/bin/env python3
"""Cost of Poisson-blending a batch of renders, per image: (a) a loop of B single-image PoissonBlender.__call__ on numpy
inputs -- what Backend.outputs() paid per call before the batched solve existed -- against (b) ONE
PoissonBlender.blend_batch on device tensors.  Shapes: 256x256 with B = 16 (outputs()), 512x512 with B = 8 (configs[2]).

Mode (a) uses nothing newer than PoissonBlender.__call__, so this script also runs on a checkout that predates blend_batch:

    python tools/blend_batch_time.py --mode single --out parent.json          (on the older checkout: the yardstick)
    python tools/blend_batch_time.py --parent parent.json                     (here: (a) and (b) alternating in one process)

Both shapes are warmed up, every figure is the wall time of work that ends in a device synchronise (the single-image call
downloads its result; the batch is followed by torch.cuda.synchronize), repeated --reps times; median, min and max are
reported in ms per image.  Writes profiles/blend_batch.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctrlhair_amd import lib, procedural as P                       # noqa: E402
from ctrlhair_amd.blending import PoissonBlender                    # noqa: E402

SHAPES = ((256, 16), (512, 8))


def inputs(S, B, seed=100):
    """The seeded images of tests/test_poisson.py::_inputs, a different hair ellipse per image; masks are the SOLVE masks."""
    ys, xs = np.mgrid[0:S, 0:S]
    src, tgt, mask = [], [], []
    for i in range(B):
        rng = np.random.default_rng(seed + i)
        s = ((P.synthetic_images(1, S, seed=seed + i)[0].transpose(1, 2, 0) * 0.5 + 0.5) * 247 + 4).astype(np.uint8)
        t = np.clip(s.astype(np.int32) + rng.integers(-25, 26, s.shape), 4, 251).astype(np.uint8)
        cy, cx = (0.3 + 0.01 * i) * S, (0.5 - 0.01 * i) * S
        ry, rx = (0.28 - 0.008 * i) * S, (0.33 - 0.008 * i) * S
        hair = ((ys - cy) ** 2 / ry ** 2 + (xs - cx) ** 2 / rx ** 2 <= 1).astype(np.uint8)
        src.append(s)
        tgt.append(t)
        mask.append(1 - hair)
    return np.stack(src), np.stack(tgt), np.stack(mask)


def stats(ms, B):
    per = [t / B for t in ms]
    return {'median_ms_per_image': round(statistics.median(per), 4), 'min_ms_per_image': round(min(per), 4),
            'max_ms_per_image': round(max(per), 4), 'reps': len(per)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', choices=('both', 'single'), default='both')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent', help='JSON written by --mode single on the parent checkout; merged into the result')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'blend_batch.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('blend_batch_time.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    blender = PoissonBlender(lib.Handle(0), dev)
    batched = a.mode == 'both'
    if batched and not hasattr(blender, 'blend_batch'):
        raise SystemExit('this checkout has no PoissonBlender.blend_batch: use --mode single')
    result = {'device': torch.cuda.get_device_name(0), 'max_iters': blender.max_iters, 'rel_tol': blender.rel_tol, 'shapes': {}}
    for S, B in SHAPES:
        src, tgt, mask = inputs(S, B)
        dsrc, dtgt, dmask = (torch.from_numpy(x).to(dev) for x in (src, tgt, mask))

        def single():
            outs, its = [], []
            for i in range(B):
                outs.append(blender(src[i], tgt[i], mask[i]))
                its.append(int(blender.last_iters))
            return outs, its

        def batch():
            out = blender.blend_batch(dsrc, dtgt, dmask)
            torch.cuda.synchronize()
            return out

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t0) * 1e3, r

        for _ in range(3):                  # warm-up of this shape: code objects, workspace, pinned staging
            outs, its = single()
            if batched:
                bout = batch()
        entry = {'B': B, 'iterations': its}
        if batched:
            same = all(np.array_equal(bout[i].cpu().numpy(), outs[i]) for i in range(B))
            entry.update(batch_iterations=[int(v) for v in blender.last_iters], batch_bit_identical_to_single=bool(same))
        ta, tb = [], []
        for _ in range(a.reps):             # alternate the two, so that both see the same machine
            ta.append(timed(single)[0])
            if batched:
                tb.append(timed(batch)[0])
        entry['single_loop_numpy'] = stats(ta, B)
        if batched:
            entry['batch_device'] = stats(tb, B)
            entry['speedup_vs_single_loop_same_build'] = round(entry['single_loop_numpy']['median_ms_per_image'] /
                                                               entry['batch_device']['median_ms_per_image'], 3)
        result['shapes'][f'{S}x{S}'] = entry
        print(f'{S}x{S} B={B}:', json.dumps(entry))
    if a.parent:
        with open(a.parent) as f:
            parent = json.load(f)
        for key, entry in result['shapes'].items():
            p = parent['shapes'][key]['single_loop_numpy']
            entry['parent_single_loop_numpy'] = p
            entry['parent_iterations'] = parent['shapes'][key]['iterations']
            if 'batch_device' in entry:
                gain = p['median_ms_per_image'] - entry['batch_device']['median_ms_per_image']
                spread = p['max_ms_per_image'] - p['min_ms_per_image']
                entry['speedup_vs_parent'] = round(p['median_ms_per_image'] / entry['batch_device']['median_ms_per_image'], 3)
                entry['gain_ms_per_image'] = round(gain, 4)
                entry['parent_spread_ms_per_image'] = round(spread, 4)
                entry['gain_exceeds_parent_spread'] = bool(gain > spread)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
