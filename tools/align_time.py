"""Times the face alignment per photo -> profiles/face_align.json.  For each fixture branch (tests/align_oracle.py CASES) at 256 and
1024 px: device time of the composite ch_face_align call (hipEvents around it, photo already on the device), host time of
align_plan, and the host oracle (Pillow / numpy / scipy) in the same session; median (min - max) of --repeats runs.  Also checks
that the device result equals the oracle's, so the timed thing is the right thing.

    python tools/align_time.py [--repeats 20] [--out profiles/face_align.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'face_align.json'))
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import alignment as A
    from ctrlhair_amd import lib
    from tests import align_oracle as O
    aligner = A.FaceAligner(lib.Handle(0), torch.device('cuda', 0))
    rows = []
    for name in O.CASES:
        photo, lm, _, _ = O.case_inputs(name)
        dev_photo = torch.from_numpy(photo).cuda()
        for S in (256, 1024):
            plan = A.align_plan(lm, photo.shape[0], photo.shape[1], S)
            want = O.run_plan(photo, plan)
            got = aligner.run_plan(dev_photo, plan)                 # warm-up: builds the Lanczos tables, sizes the workspace
            torch.cuda.synchronize()
            exact = bool(np.array_equal(got.cpu().numpy(), want))
            dev, host_plan, oracle = [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                plan = A.align_plan(lm, photo.shape[0], photo.shape[1], S)
                host_plan.append((time.perf_counter() - t0) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                aligner.run_plan(dev_photo, plan)
                e1.record()
                e1.synchronize()
                dev.append(e0.elapsed_time(e1))
                t0 = time.perf_counter()
                O.run_plan(photo, plan)
                oracle.append((time.perf_counter() - t0) * 1e3)
            row = {'case': name, 'photo': [photo.shape[1], photo.shape[0]], 'output_size': S, 'transform_size': 4096,
                   'shrink': plan['shrink'], 'cropped': plan['cropped'], 'padded': plan['padded'], 'equals_host_oracle': exact,
                   'device_composite': stats(dev), 'host_plan': stats(host_plan), 'host_oracle': stats(oracle)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = {'what': 'face alignment per photo: ch_face_align on the device vs the host oracle (Pillow / numpy / scipy), one session',
           'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'cpu_threads': os.cpu_count(),
           'cpu_threads_allowed': len(os.sched_getaffinity(0)), 'rows': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    assert all(r['equals_host_oracle'] for r in rows)


if __name__ == '__main__':
    main()
