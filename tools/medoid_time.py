"""Times ch_style_medoid and writes profiles/style_medoid.json.

R = 19 segments of n codes each (n = 1 000, 8 000, 30 000; dim 512, tanh(0.4 N) codes): median (min-max) of 20 repeats of the whole
call, and the vector lane-operations per second it achieves -- 2 per pair and dimension, one subtract and one fused multiply-add --
against the MI355X's float32 vector peak of 157.3 TFLOP/s = 78.6e12 fused multiply-adds per second.  Where the n x n matrix fits
(n <= 8 000) the reference's float32 Gram arithmetic in numpy is timed on the same machine for one region and scaled to 19.  The largest
relative error of the row sums against the float64 difference-form oracle is taken over the input families of tests/test_hip_medoid.py.

    python tools/medoid_time.py [--sizes 1000 8000 30000] [--repeats 20] [--out profiles/style_medoid.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_LANE_OPS = 157.3e12 / 2          # one v_fma_f32 lane-operation counts as 2 FLOP in the 157.3 TFLOP/s vector peak
R, DIM = 19, 512


def device_codes(n_total, device, seed=0):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.tanh(0.4 * torch.randn(n_total, DIM, generator=g, device=device, dtype=torch.float32))


def time_call(sm, x, off, repeats):
    import torch
    sm.segments(x, off)                      # warm-up: workspace allocation, code object load
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sm.segments(x, off)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def reference_numpy_seconds(n, repeats=3):
    from tests import medoid_oracle as O
    x = O.tanh_codes(n, DIM, seed=1)
    best = float('inf')
    for _ in range(repeats):
        t = time.perf_counter()
        O.reference_f32(x)
        best = min(best, time.perf_counter() - t)
    return best


def max_error(sm):
    from tests import medoid_oracle as O
    worst, where = 0.0, None
    cases = [('planted', O.planted(n, d, seed=n)[0]) for n, d in ((3, 512), (127, 512), (129, 512), (257, 512), (1000, 512), (130, 4),
                                                                   (130, 12))]
    cases += [('saturated', O.saturated()), ('two_clusters', O.two_clusters())]
    for name, x in cases:
        _, sums, _ = sm.segments(x, np.array([0, len(x)], np.int64))
        s64 = O.row_sums_f64(x)
        err = float((np.abs(sums.cpu().numpy() - s64) / s64).max())
        if err > worst:
            worst, where = err, f'{name} n={len(x)} dim={x.shape[1]}'
    return worst, where


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[1000, 8000, 30000])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'style_medoid.json'))
    args = ap.parse_args()
    import torch
    from ctrlhair_amd import lib
    from ctrlhair_amd.stylestats import StyleMedoid
    dev = torch.device('cuda', 0)
    sm = StyleMedoid(lib.Handle(0), dev)
    err, where = max_error(sm)
    res = {'device': torch.cuda.get_device_name(0), 'segments': R, 'dim': DIM, 'repeats': args.repeats,
           'peak_vector_lane_ops_per_s': PEAK_LANE_OPS, 'bound_rel_error': 2e-5, 'max_rel_error_observed': err, 'max_rel_error_case': where,
           'sizes': []}
    print(f'max relative error of the row sums: {err:.3e} ({where})')
    for n in args.sizes:
        x = device_codes(R * n, dev)
        off = np.arange(R + 1, dtype=np.int64) * n
        ms = time_call(sm, x, off, args.repeats)
        med = float(np.median(ms))
        lane_ops = 2.0 * R * n * n * DIM
        row = {'n': n, 'ms_median': med, 'ms_min': float(min(ms)), 'ms_max': float(max(ms)), 'lane_ops': lane_ops,
               'lane_ops_per_s': lane_ops / (med * 1e-3), 'fraction_of_vector_peak': lane_ops / (med * 1e-3) / PEAK_LANE_OPS}
        if n <= 8000:
            sec = reference_numpy_seconds(n)
            row['reference_numpy_ms_one_region'] = sec * 1e3
            row['reference_numpy_ms_19_regions'] = sec * 1e3 * R
            row['reference_numpy_threads'] = int(os.environ.get('OMP_NUM_THREADS', '0')) or None
        res['sizes'].append(row)
        print(f'n={n}: {med:.2f} ms ({min(ms):.2f}-{max(ms):.2f}), {row["lane_ops_per_s"] / 1e12:.1f}e12 lane-ops/s = '
              f'{100 * row["fraction_of_vector_peak"]:.1f} % of vector peak'
              + (f', numpy reference {row["reference_numpy_ms_19_regions"]:.0f} ms' if n <= 8000 else ''), flush=True)
        del x
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
