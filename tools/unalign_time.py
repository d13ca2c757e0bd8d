"""Times the paste-back (ch_face_unalign) -> profiles/unalign.json.  Three shapes: one 512^2 edit into a 3000 x 4000 photo, 16 edits
of 512^2 into a 1024 x 1024 photo, and a minifying paste of a 1024^2 edit into a 600 x 700 photo.  Device time: hipEvents around the
call, inputs already on the device, median (min-max) of --repeats calls after a warm-up, one session.  Yardstick: the float64 numpy
oracle (tests/unalign_oracle.py) on this host's CPUs, once per shape.  Bytes: `out` written once and the photo read once per edit,
plus the edits -- the copy-bound floor of the call -- over the device time.

    python tools/unalign_time.py [--repeats 20] [--out profiles/unalign.json] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (photo height, width, eye centre (x, y), eye distance, angle, S, N)
SHAPES = {
    'one_512_into_3000x4000': (4000, 3000, (1500.0, 1700.0), 330.0, 6.0, 512, 1),
    'sixteen_512_into_1024x1024': (1024, 1024, (512.0, 470.0), 150.0, -5.0, 512, 16),
    'minify_1024_into_600x700': (700, 600, (300.0, 320.0), 75.0, 9.0, 1024, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unalign.json'))
    ap.add_argument('--no-oracle', action='store_true')
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import alignment as AL
    from tests import align_oracle as AO
    from tests import unalign_oracle as UO
    al = AL.FaceAligner(device='cuda:0')
    rows = {}
    for name, (H, W, centre, eye, angle, S, N) in SHAPES.items():
        photo = AO.make_photo(1, H, W)
        plan = AL.align_plan(AO.make_landmarks(2, centre, eye, angle), H, W, S, max(S, 1024))
        pu = AL.unalign_plan(plan, H, W)
        edits = np.stack([AO.make_photo(10 + n, S, S) for n in range(N)])
        dp, de = torch.from_numpy(photo).cuda(), torch.from_numpy(edits).cuda()
        for _ in range(3):
            out = al.paste_back(dp, de, pu)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = al.paste_back(dp, de, pu)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        x0, y0, x1, y1 = pu['bbox']
        nbytes = N * 2 * H * W * 3 + N * S * S * 3
        row = {'photo': [H, W], 'S': S, 'N': N, 'scale': pu['scale'], 'bbox': list(pu['bbox']),
               'bbox_share_of_photo': (x1 - x0) * (y1 - y0) / (H * W), 'device_ms': {'median': float(np.median(ms)), 'min': min(ms), 'max': max(ms)},
               'floor_bytes': nbytes, 'achieved_GBps': nbytes / (float(np.median(ms)) * 1e-3) / 1e9}
        if not args.no_oracle:
            t = time.perf_counter()
            ref = UO.paste_back(photo, edits, pu)
            row['oracle_cpu_s'] = time.perf_counter() - t
            d = np.abs(out.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
            row['vs_oracle'] = {'max': int(d.max()), 'share_inside_bbox': float((d[:, y0:y1, x0:x1].max(axis=-1) > 0).mean())}
        rows[name] = row
        print(name, json.dumps(row), flush=True)
    res = {'what': 'paste-back: ch_face_unalign on the device vs the float64 numpy oracle on the host CPUs, one session',
           'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'shapes': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
