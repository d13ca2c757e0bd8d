"""Times the matte paste-back (ch_face_unalign_matte) -> profiles/matte.json.  The three shapes of tools/unalign_time.py with a
hair-like weight map (a blob with a wavy outline and a few holes, 255 / 0): per shape the matte call at the default radius
(alignment.matte_params) and the plain ch_face_unalign call with the same weight beside it; on the 3000 x 4000 shape also r = 2 and
r = 32, whose ratio says whether the cost depends on the radius.  Device time: hipEvents around the call, inputs already on the
device, median (min-max) of --repeats calls after a warm-up, one session.  Yardstick: the float64 numpy oracle
(tests/matte_oracle.py) on this host's CPUs, once per shape, with the accuracy of alpha and of the composite against it.

Bytes, from the shapes (n = pixels of bbox, P = H W 3, N edits of S^2 3 bytes):
  floor    every plane read and written once: copy P read + P N written (bbox included, as in unalign_time.py), edits read, weight
           read, p8 written and read (2 n), photo inside bbox read by three passes (9 n), (a, b) written and read (32 n), alpha
           written and read (8 n)
  issued   what the box passes load: each sliding step reads the entering and the leaving row, a strip of 256 columns has
           256 - 2 r outputs, and a segment warms up on 2 r + 1 rows; most of the re-reads hit L2
The share of the measured HBM copy rate is floor bytes over the device time.

    python tools/matte_time.py [--repeats 20] [--out profiles/matte.json] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.unalign_time import SHAPES  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X (8.0 TB/s specified)
BIG = 'one_512_into_3000x4000'


def hair_weight(S, seed=0):
    """A hair-like region at S x S: a blob whose radius varies with the angle (a wavy outline), a face-sized hole below its centre
    and a few strands cut out, 255 / 0."""
    rng = np.random.RandomState(seed)
    j, i = np.mgrid[0:S, 0:S]
    u, v = (i + 0.5) / S - 0.5, (j + 0.5) / S - 0.42
    th, rad = np.arctan2(v, u), np.hypot(u, v)
    edge = 0.36 + sum(a * np.sin(k * th + p) for k, a, p in zip((3, 7, 17, 41), (0.03, 0.02, 0.012, 0.006), rng.uniform(0, 6.28, 4)))
    w = rad < edge
    w &= ~(((u / 0.17) ** 2 + ((v - 0.12) / 0.24) ** 2) < 1)                  # the face
    w &= ~((np.abs(np.sin(40 * u + 9 * v)) < 0.06) & (v > 0.1))               # gaps between strands
    return (w * 255).astype(np.uint8)


def box_pass_issued_rows(bw, bh, r):
    """(strips, rows loaded per column of a strip summed over segments) of the kernels' cut of a bw x bh domain (face_matte.hip)."""
    outw = 256 - 2 * r
    nbx = -(-bw // outw)
    seg = 128
    while seg > 16 and seg > r and nbx * -(-bh // seg) < 1024:
        seg //= 2
    rows = 0
    for ys in range(0, bh, seg):
        ye = min(ys + seg, bh)
        rows += min(ys + r, bh - 1) - max(ys - r, 0) + 1
        rows += sum((y + r + 1 < bh) + (y - r >= 0) for y in range(ys, ye - 1))
    return nbx, rows, seg


def byte_counts(H, W, S, N, bbox, r):
    n = (bbox[2] - bbox[0]) * (bbox[3] - bbox[1])
    bw, bh = bbox[2] - bbox[0], bbox[3] - bbox[1]
    P = H * W * 3
    floor = P + P * N + N * S * S * 3 + S * S + 2 * n + 9 * n + 32 * n + 8 * n
    nbx, rows, seg = box_pass_issued_rows(bw, bh, r)
    cols = min(nbx * 256, bw + 2 * r * nbx)                                   # columns that lie inside the domain, halo included
    issued = P + P * N + N * S * S * 3 + S * S + n + cols * rows * (4 + 16) + 16 * n + 3 * n + 4 * n + (4 + 3) * n
    return {'floor_bytes': int(floor), 'issued_bytes': int(issued), 'rows_per_segment': seg, 'strips': nbx}


def timed(fn, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median': float(np.median(ms)), 'min': min(ms), 'max': max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matte.json'))
    ap.add_argument('--no-oracle', action='store_true')
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import alignment as AL
    from tests import align_oracle as AO
    from tests import matte_oracle as MO
    al = AL.FaceAligner(device='cuda:0')
    rows = {}
    for name, (H, W, centre, eye, angle, S, N) in SHAPES.items():
        photo = AO.make_photo(1, H, W)
        plan = AL.align_plan(AO.make_landmarks(2, centre, eye, angle), H, W, S, max(S, 1024))
        pu = AL.unalign_plan(plan, H, W)
        edits = np.stack([AO.make_photo(10 + n, S, S) for n in range(N)])
        weight = hair_weight(S)
        dp, de, dw = torch.from_numpy(photo).cuda(), torch.from_numpy(edits).cuda(), torch.from_numpy(weight).cuda()
        r0, eps = AL.matte_params(True, pu['scale'])
        row = {'photo': [H, W], 'S': S, 'N': N, 'scale': pu['scale'], 'bbox': list(pu['bbox']), 'eps': eps, 'default_radius': r0,
               'weight_hair_share': float((weight > 0).mean()),
               'plain_unalign_ms': timed(lambda: al.paste_back(dp, de, pu, weight=dw), args.repeats), 'matte': {}}
        for r in ([r0, 2, 32] if name == BIG else [r0]):
            m = {'radius': r, 'eps': eps}
            t = timed(lambda: al.paste_back(dp, de, pu, weight=dw, matte=m), args.repeats)
            b = byte_counts(H, W, S, N, pu['bbox'], r)
            rate = b['floor_bytes'] / (t['median'] * 1e-3)
            row['matte'][f'r{r}'] = dict(b, device_ms=t, floor_GBps=rate / 1e9, share_of_hbm_copy_rate=rate / HBM_COPY_BYTES_PER_S)
        if name == BIG:
            row['r32_over_r2'] = row['matte']['r32']['device_ms']['median'] / row['matte']['r2']['device_ms']['median']
        if not args.no_oracle:
            out, alpha = al.paste_back(dp, de, pu, weight=dw, matte={'radius': r0, 'eps': eps}, return_alpha=True)
            t = time.perf_counter()
            ref, ref_alpha = MO.paste_back_matte(photo, edits, pu, weight, None, r0, eps)
            row['oracle_cpu_s'] = time.perf_counter() - t
            x0, y0, x1, y1 = pu['bbox']
            d = np.abs(out.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
            row['vs_oracle'] = {'alpha_max_abs': float(np.abs(alpha.cpu().numpy().astype(np.float64) - ref_alpha).max()),
                                'max': int(d.max()), 'share_inside_bbox': float((d[:, y0:y1, x0:x1].max(axis=-1) > 0).mean())}
        rows[name] = row
        print(name, json.dumps(row), flush=True)
    res = {'what': 'matte paste-back: ch_face_unalign_matte on the device beside ch_face_unalign with the same weight, and the float64 numpy '
                   'oracle on the host CPUs, one session',
           'command': 'python tools/matte_time.py --repeats %d' % args.repeats,
           'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'hbm_copy_bytes_per_s': HBM_COPY_BYTES_PER_S,
           'note': 'the same buffers are used by every repeat and by consecutive passes: the planes of one call (189 MB for the '
                   'largest shape) fit the 256 MiB Infinity Cache, so part of the traffic never reaches HBM and the share flatters the HBM figure',
           'shapes': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
