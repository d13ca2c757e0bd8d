"""Times the device PNG decoder against the path it replaces -> profiles/png_decode.json.  One session, after warm-up, median (min - max)
of --repeats runs, the two sides alternating in one loop.

  inputs      256 x 256 and 1024 x 1024 RGB crops (procedural: smooth colour fields, soft edges, sensor-like noise) and 256 x 256 / 512 x 512
              label maps (discs of labels), 16 different images each; every one written once by Pillow at its default level and once by
              pngenc.PngEncoder; batches of 16 and of 256 (the 16 files 16 times over).  Files are read from the page cache on both sides.
  yardstick   the host path: dataset.read_rgb / read_gray per file (Pillow), np.stack, one upload of the stacked batch, synchronise
  device      file read + pngdec.parse_png (container walk, CRC-32) | packing + the one upload of the compressed bytes | ch_png_decode
              (device events around the one call: inflate + unfilter) | total; MB/s of filtered bytes (H * (1 + W * C) per image) over
              the call's time, in aggregate and per stream (aggregate / N: the streams run side by side)
  rgb job     dataset.hair_color_stats over 256 files of 256 x 256 (and their 256 x 256 label maps), batch 16 and batch 256, decode='host'
              and decode='device' alternating
The split of the call into its two kernels comes from a kernel trace in a run of its own (--kernels-only under rocprofv3 --kernel-trace
--stats): device events cannot be placed between launches that one C call enqueues.  --kernel-stats CSV adds that trace's per-kernel
table to the JSON.

    python tools/png_decode_time.py [--repeats 20] [--out profiles/png_decode.json] [--kernels-only] [--kernel-stats kernel_stats.csv]
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def spread(ms):
    ms = sorted(ms)
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}


def photo(H, W, seed=0):
    """A photo-like uint8 [H,W,3]: smooth colour fields, soft edges and sensor-like noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    out = np.empty((H, W, 3), np.float32)
    for c in range(3):
        f = rng.uniform(2, 9, 4) / np.float32(max(H, W))
        out[:, :, c] = 128 + 70 * np.sin(f[0] * yy + f[1] * xx + c) + 40 * np.tanh(8 * np.sin(f[2] * yy * 3) * np.cos(f[3] * xx * 3))
    out += rng.normal(0, 2.5, out.shape).astype(np.float32)
    return np.clip(out, 0, 255).astype(np.uint8)


def hair_label(size, seed):
    """A label map with a hair (13) region, like the masks job's output."""
    import png_oracle as PO
    lab = PO.label_map(size, 18, seed)
    yy, xx = np.mgrid[:size, :size]
    lab[(yy - size // 3) ** 2 + (xx - size // 2) ** 2 < (size // 4) ** 2] = 13
    return lab


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true', help='only the ch_png_decode calls (for a kernel trace)')
    ap.add_argument('--kernel-stats', default=None, help="a rocprofv3 --stats kernel table (CSV) of a --kernels-only run, added to the JSON")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_decode.json'))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from ctrlhair_amd import colorstats as CS
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import lib, pngdec, pngenc
    dev = torch.device('cuda', 0)
    handle = lib.Handle(0)
    dec, enc = pngdec.PngDecoder(handle, dev), pngenc.PngEncoder(handle, dev)
    work = tempfile.mkdtemp(prefix='png_decode_time_')
    ev = lambda: torch.cuda.Event(enable_timing=True)

    kinds = [('rgb256', 3, 256), ('rgb1024', 3, 1024), ('label256', 1, 256), ('label512', 1, 512)]
    rows = []
    for kind, C, S in kinds:
        imgs = np.stack([photo(S, S, k) if C == 3 else hair_label(S, k) for k in range(16)])
        for writer in ('pillow', 'encoder'):
            d = os.path.join(work, f'{kind}_{writer}')
            os.makedirs(d)
            paths = [os.path.join(d, f'{k:02d}.png') for k in range(16)]
            if writer == 'pillow':
                for p, im in zip(paths, imgs):
                    Image.fromarray(im).save(p)
            else:
                enc.write(paths, torch.from_numpy(imgs).to(dev))
            for B in (16, 256):
                batch = paths * (B // 16)
                host_read = D.read_rgb if C == 3 else D.read_gray
                filtered_bytes = B * S * (1 + S * C)
                row = {'input': kind, 'writer': writer, 'batch': B, 'H': S, 'W': S, 'C': C, 'file_bytes': sum(os.path.getsize(p) for p in batch),
                       'filtered_bytes': filtered_bytes}
                t = {k: [] for k in ('host_total', 'dev_read_parse', 'dev_upload', 'dev_kernels', 'dev_total')}
                want = None
                for rep in range(-2, args.repeats):                                           # two warm-up rounds
                    if not args.kernels_only:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        x = torch.from_numpy(np.stack([host_read(p) for p in batch])).to(dev)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        want = x
                    t2 = time.perf_counter()
                    streams = []
                    for p in batch:
                        with open(p, 'rb') as f:
                            streams.append(pngdec.parse_png(f.read())[3])
                    t3 = time.perf_counter()
                    up = dec.upload(streams)
                    torch.cuda.synchronize()
                    t4 = time.perf_counter()
                    e0, e1 = ev(), ev()
                    e0.record()
                    img, status = dec.launch(up, S, S, C)
                    e1.record()
                    torch.cuda.synchronize()
                    t5 = time.perf_counter()
                    if rep < 0:
                        assert int(status.abs().sum()) == 0
                        if want is not None:
                            assert torch.equal(img.reshape(want.shape), want), (kind, writer, B)
                        continue
                    if not args.kernels_only:
                        t['host_total'].append((t1 - t0) * 1e3)
                    t['dev_read_parse'].append((t3 - t2) * 1e3)
                    t['dev_upload'].append((t4 - t3) * 1e3)
                    t['dev_kernels'].append(e0.elapsed_time(e1))
                    t['dev_total'].append((t5 - t2) * 1e3)
                row.update({k: spread(v) for k, v in t.items() if v})
                k_ms = row['dev_kernels']['median_ms']
                row['filtered_MB_per_s_aggregate'] = round(filtered_bytes / 1e6 / (k_ms / 1e3), 1)
                row['filtered_MB_per_s_per_stream'] = round(filtered_bytes / 1e6 / (k_ms / 1e3) / B, 2)
                if not args.kernels_only:
                    h, dv = row['host_total'], row['dev_total']
                    row['verdict'] = ('device faster' if dv['max_ms'] < h['min_ms'] else 'host faster' if dv['min_ms'] > h['max_ms'] else
                                      'within the spread')
                rows.append(row)
                print(json.dumps(row), flush=True)

    job = {}
    if not args.kernels_only:
        root = os.path.join(work, 'tree')
        img_dir, lab_dir = os.path.join(root, 'ds', 'images_256'), os.path.join(root, 'ds', 'label')
        os.makedirs(img_dir)
        os.makedirs(lab_dir)
        for k in range(256):
            Image.fromarray(photo(256, 256, 100 + k % 32)).save(os.path.join(img_dir, f'{k:03d}.png'))
            D.write_label_png(os.path.join(lab_dir, f'{k:03d}.png'), hair_label(256, k % 32))
        stats = CS.HairColorStats(handle, dev)
        for B in (16, 256):
            t = {'host': [], 'device': []}
            for rep in range(-1, args.repeats):
                for mode in ('host', 'device'):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = D.hair_color_stats(stats, img_dir, lab_dir, os.path.join(root, f'out_{mode}'), 'ds', ('rgb',), B, decode=mode)
                    torch.cuda.synchronize()
                    if rep >= 0:
                        t[mode].append((time.perf_counter() - t0) * 1e3)
                    assert len(res['rgb']) == 256
            h, dv = spread(t['host']), spread(t['device'])
            job[f'batch{B}'] = {'files': 256, 'host': h, 'device': dv, 'images_per_s_host': round(256e3 / h['median_ms'], 1),
                                'images_per_s_device': round(256e3 / dv['median_ms'], 1),
                                'verdict': 'device faster' if dv['max_ms'] < h['min_ms'] else 'host faster' if dv['min_ms'] > h['max_ms'] else
                                'within the spread'}
            print(json.dumps({f'rgb_job_batch{B}': job[f'batch{B}']}), flush=True)

    out = {'what': 'ch_png_decode (one upload of the compressed bytes, inflate + unfilter on the device) against dataset.read_rgb / read_gray per '
                   'file + one upload of the stacked batch; median (min - max), the two sides alternating; one session',
           'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'inputs': rows, 'rgb_job_256_files': job}
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            out['kernel_trace'] = [r for r in csv.DictReader(f) if 'png_' in r.get('Name', '')]
    if not args.kernels_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
