"""Meshing for the hair-shape transfer, host against device: writes profiles/delaunay_batch.json.

One session on the GPU, the fixture landmark sets (tests/golden/warp_cases.npz) cycled to B = 1 and B = 16, 20 repeats each after
3 warm-up calls, every figure per pair as median (min - max) in ms:
  (a) host_build_mesh          warping.build_mesh (scipy / Qhull + canonical form) alone, host clock
  (b) delaunay_batch           ch_delaunay_batch alone on points already on the device, device events
  (c) warp_batch_host_mesher   the whole warp_batch(mesher='host') call, host clock around a synchronised call
  (d) warp_batch_device_mesher the whole warp_batch(mesher='device') call, the same way
  (e) exact_fraction           incircle tests the float64 filter passed on to the integer evaluation / all incircle tests
The claim is that (d) is faster per pair than (c) at B = 16 by more than the spread of both: max (d) < min (c).  The tool exits
non-zero otherwise.

    python tools/mesh_time.py [--repeats 20] [--out profiles/delaunay_batch.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms, per):
    a = np.asarray(ms, np.float64) / per
    return {'median': float(np.median(a)), 'min': float(a.min()), 'max': float(a.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'delaunay_batch.json'))
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import warping as W
    if not torch.cuda.is_available():
        raise SystemExit('mesh_time.py measures on the GPU; none is visible')
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'warp_cases.npz'))
    warper = W.MaskWarper(device='cuda:0')
    dev = warper.device
    res = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'unit': 'ms per pair: median, min, max'}
    for B in (1, 16):
        sel = [k % 4 for k in range(B)]
        hl, fl = z['hair_lm'][sel], z['face_lm'][sel]
        hair, face = torch.from_numpy(z['hair_labels'][sel]).to(dev), torch.from_numpy(z['face_labels'][sel]).to(dev)
        nodes = [W.build_nodes(h, f)[0] for h, f in zip(hl, fl)]
        V, counts, _ = W.build_points_batch(hl, fl)
        Vd = torch.from_numpy(V).to(dev)

        def host_mesh():
            for nd in nodes:
                W.build_mesh(nd)

        def wall(fn):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t) * 1e3

        def events(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        arms = {
            'host_build_mesh_ms_per_pair': lambda: wall(host_mesh),
            'delaunay_batch_ms_per_pair': lambda: events(lambda: warper._delaunay(Vd, counts)),
            'warp_batch_host_mesher_ms_per_pair': lambda: wall(lambda: warper.warp_batch(hair, face, hl, fl, mesher='host')),
            'warp_batch_device_mesher_ms_per_pair': lambda: wall(lambda: warper.warp_batch(hair, face, hl, fl, mesher='device')),
        }
        times = {k: [] for k in arms}
        for rep in range(-3, args.repeats):              # the arms alternate inside every repeat: they share the machine's noise
            for k, fn in arms.items():
                t = fn()
                if rep >= 0:
                    times[k].append(t)
        assert int(warper.last_mesh_status.abs().sum()) == 0
        warper._delaunay(Vd, counts)
        cnt = warper.delaunay_counters(B).sum(0)
        r = {k: stats(v, B) for k, v in times.items()}
        r['incircle_tests_per_set'] = float(cnt[0]) / B
        r['exact_fraction'] = float(cnt[1]) / float(cnt[0])
        res[f'B{B}'] = r
        for k, v in r.items():
            print(f'B = {B:2d}  {k:40s}', v if not isinstance(v, dict) else f"{v['median']:.3f} ({v['min']:.3f} - {v['max']:.3f})")
    c, d = res['B16']['warp_batch_host_mesher_ms_per_pair'], res['B16']['warp_batch_device_mesher_ms_per_pair']
    res['device_mesher_faster_at_B16'] = bool(d['max'] < c['min'])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    if not res['device_mesher_faster_at_B16']:
        raise SystemExit(f"the device mesher is not faster per pair at B = 16 beyond the spread: (d) max {d['max']:.3f} ms, (c) min {c['min']:.3f} ms")


if __name__ == '__main__':
    main()
