#!/usr/bin/env python3
"""Hair colour statistics: kernel times (hipEvents), HairEditor.get_hair_color latency, and the throughput of the colorvar
dataset job against the numpy / CPU path, with the PNG decode that bounds both.  Prints one JSON line per measurement.

    python tools/colorstats_bench.py [--images 256] [--procs 16] [--reps 20]
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def _cpu_one(args):
    """The reference's per-image work on the host (script_get_color_var_label.py:48-86): decode, nearest resize, erosion,
    statistics, pickle."""
    import pickle
    from ctrlhair_amd import dataset as D
    from tests import colorstats_ref as R
    img_path, lab_path, out_path = args
    img = D.read_rgb(img_path)
    pts = img[R.hair_mask(D.read_gray(lab_path), img.shape[0]).astype(bool)]
    v = R.color_var(pts)
    if v is not None:
        with open(out_path, 'wb') as f:
            pickle.dump(v, f)


def _decode_one(args):
    from ctrlhair_amd import dataset as D
    D.read_rgb(args[0])
    D.read_gray(args[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--procs', type=int, default=16, help='CPU processes of the numpy path (the CPU quota of the GPU box)')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from tests import colorstats_ref as R

    tmp = tempfile.mkdtemp(prefix='colorstats_bench_')
    ds = 'synth'
    img_dir, lab_dir = os.path.join(tmp, ds, 'images_256'), os.path.join(tmp, ds, 'label')
    os.makedirs(img_dir)
    os.makedirs(lab_dir)
    rng = np.random.default_rng(0)
    for i in range(args.images):
        img, lab = R.synth_image_and_labels(rng, 256, 512, 'blob')
        Image.fromarray(img).save(os.path.join(img_dir, f'{i:05d}.png'))
        D.write_label_png(os.path.join(lab_dir, f'{i:05d}.png'), lab)
    names = D.list_images(img_dir)
    work = [(os.path.join(img_dir, n), os.path.join(lab_dir, n), os.path.join(tmp, 'cpu_' + n[:-4] + '.pkl')) for n in names]

    # ---- host legs first (spawned workers; no process has opened the GPU yet) ----
    ctx = mp.get_context('spawn')
    with ctx.Pool(args.procs) as pool:
        pool.map(_decode_one, work[:args.procs])                 # worker start-up outside the timings
        t0 = time.perf_counter()
        pool.map(_decode_one, work, chunksize=4)
        t_dec = time.perf_counter() - t0
        t0 = time.perf_counter()
        pool.map(_cpu_one, work, chunksize=4)
        t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    for w in work:
        _decode_one(w)
    t_dec1 = time.perf_counter() - t0
    emit(metric='png_decode', procs=args.procs, images_per_s=args.images / t_dec, single_process_images_per_s=args.images / t_dec1)
    emit(metric='colorvar_job_cpu_numpy', procs=args.procs, images_per_s=args.images / t_cpu)

    # ---- device legs ----
    import torch
    from ctrlhair_amd import lib
    from ctrlhair_amd.colorstats import HairColorStats
    dev = torch.device('cuda', 0)
    cs = HairColorStats(lib.Handle(0), dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    B = 64
    imgs = torch.from_numpy(rng.integers(0, 256, (B, 256, 256, 3), dtype=np.uint8)).to(dev)
    labs = torch.from_numpy(np.stack([R.synth_image_and_labels(rng, 256, 512, 'blob')[1] for _ in range(B)])).to(dev)
    mask = cs.erode(labs, 256)
    t_er = timed(lambda: cs.erode(labs, 256))
    t_su = timed(lambda: cs.mask_sums(imgs, mask))
    t_both = timed(lambda: cs.mask_sums(imgs, cs.erode(labs, 256)))
    mb = (B * 512 * 512 + B * 256 * 256 * 4) / 1e6
    emit(metric='erode_sums_b64_256', erode_ms=t_er, sums_ms=t_su, erode_plus_sums_ms=t_both, images_per_s=B / t_both * 1e3,
         min_traffic_MB=mb, GB_per_s=mb / t_both)
    big = torch.from_numpy(rng.integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)).to(dev)
    lab1 = labs[:1]
    emit(metric='get_hair_color_device_part_1024', resize_ms=timed(lambda: cs.resize(big, 1024)),
         erode_ms=timed(lambda: cs.erode(lab1, 1024)),
         resize_erode_sums_ms=timed(lambda: cs.mask_sums(cs.resize(big, 1024), cs.erode(lab1, 1024))))

    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import HairEditor, procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, 16)
    he = HairEditor(True, True, weights=w, device=0)
    img = ((P.synthetic_images(1, 256, seed=3)[0].transpose(1, 2, 0) * 0.5 + 0.5) * 255).astype(np.uint8)
    for _ in range(3):
        he.get_hair_color(img)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        he.get_hair_color(img)
        ts.append((time.perf_counter() - t0) * 1e3)
    emit(metric='get_hair_color_latency_1024', ms_median=float(np.median(ts)), ms_min=float(np.min(ts)))

    out = os.path.join(tmp, 'out')
    D.hair_color_stats(cs, img_dir, lab_dir, out, ds, ('colorvar',), batch=64)      # warm-up
    t0 = time.perf_counter()
    D.hair_color_stats(cs, img_dir, lab_dir, out, ds, ('colorvar',), batch=64)
    t_job = time.perf_counter() - t0
    emit(metric='colorvar_job_gpu', procs=1, batch=64, images_per_s=args.images / t_job,
         decode_share=min(1.0, t_dec1 / t_job), cpu_16proc_images_per_s=args.images / t_cpu,
         bound='png decode + file writes on one host process' if t_dec1 / t_job > 0.5 else 'host-side finishing / launches')
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
