"""Times the hair-shape mask warp on the GPU and measures its ARAP error -> profiles/warp_batch.json (--out).

Per pair, median (min - max) of 20 repeats after warm-up, hipEvents around the enqueue (mesh upload included): one pair and
B = 16, whole call and render + sample alone (U given); the ARAP solve is estimated as the difference of the two medians
(both contain the same host packing and uploads).  Exits non-zero unless B = 16 is cheaper per pair than one pair.  Host meshing (scipy Delaunay) and the
host oracle (tests/warp_oracle.py, the only baseline that runs here: the reference's tool chain needs binaries that do not
exist) are timed with perf_counter.  `arap_max_dU_px` = max |U_gpu - U_oracle| over the fixture meshes: tests/test_hip_warp.py
asserts 4x that."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    v = np.asarray(v, np.float64)
    return {'median': float(np.median(v)), 'min': float(v.min()), 'max': float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_batch.json'))
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import warping as W
    from tests import warp_oracle as O
    from tests.warp_cases import cases, triangle_meshes
    cs = cases()
    warper = W.MaskWarper(device='cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'unit': 'ms per pair',
           'mesh': [{'vertices': int(len(c['V'])), 'triangles': int(len(c['F']))} for c in cs]}

    t = []
    for c in cs * 3:
        t0 = time.perf_counter()
        W.build_mesh(W.build_nodes(c['hair_lm'], c['face_lm'])[0])
        t.append((time.perf_counter() - t0) * 1e3)
    res['host_meshing'] = stat(t)

    dU, t, oracle_U = [], [], []
    for c in cs:
        t0 = time.perf_counter()
        lab, _, U = O.warp(c['hair'], c['face'], c['V'], c['F'], c['b'], c['bc'])
        t.append((time.perf_counter() - t0) * 1e3)
        oracle_U.append(U)
        g = warper.warp_with_mesh(c['hair'], c['face'], c['V'], c['F'], c['b'], c['bc'], return_U=True)['U'].cpu().numpy()
        dU.append(float(np.linalg.norm(g - O.arap(c['V'], c['F'], c['b'], c['bc']), axis=1).max()))
    res['host_oracle'] = stat(t)
    for c in triangle_meshes():        # the meshes Triangle itself made for pairs 0 and 1: part of the bound, not of the timing
        g = warper.warp_with_mesh(c['hair'], c['face'], c['V'], c['F'], c['b'], c['bc'], return_U=True)['U'].cpu().numpy()
        dU.append(float(np.linalg.norm(g - O.arap(c['V'], c['F'], c['b'], c['bc']), axis=1).max()))
    res['arap_dU_px_per_case'] = dU
    res['arap_max_dU_px'] = max(dU)

    for B in (1, 16):
        sel = [cs[k % 4] for k in range(B)]
        hair = torch.from_numpy(np.stack([c['hair'] for c in sel])).cuda()
        face = torch.from_numpy(np.stack([c['face'] for c in sel])).cuda()
        meshes = [(c['V'], c['F'], c['b'], c['bc']) for c in sel]
        Us = [oracle_U[k % 4] for k in range(B)]
        for name, kw in (('whole_call', {}), ('render_sample', {'U': Us})):
            t = []
            for r in range(args.reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                warper.warp_meshes(hair, face, meshes, **kw)
                e1.record()
                e1.synchronize()
                if r >= 3:
                    t.append(e0.elapsed_time(e1) / B)
            res[f'B{B}_{name}'] = stat(t)
        res[f'B{B}_arap_estimate_median'] = res[f'B{B}_whole_call']['median'] - res[f'B{B}_render_sample']['median']
    res['batch16_cheaper_per_pair_than_single'] = res['B16_whole_call']['median'] < res['B1_whole_call']['median']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    if not res['batch16_cheaper_per_pair_than_single']:
        sys.exit('the B = 16 call costs no less per pair than the single call')


if __name__ == '__main__':
    main()
