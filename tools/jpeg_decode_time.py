"""Times the device JPEG decoder against the path it replaces -> profiles/jpeg_decode.json.  One session, after warm-up, median (min - max)
of --repeats runs, the two sides alternating in one loop.

  inputs      photo-like images (procedural: smooth colour fields, soft edges, sensor-like noise) saved by Pillow at quality 90, 4:2:0:
              one of 3000 x 4000, one of 1600 x 2000, one crop of 1024 x 1024, 16 crops of 256 x 256.  Files are in memory on both sides.
  yardstick   what the parent commit does: Pillow decode per file (Image.open(...).convert('RGB')), np.stack, one upload of the pixels,
              synchronise
  device      jpegdec.parse_jpeg (the marker walk) | packing + the one upload of the compressed bytes and tables | ch_jpeg_decode (device
              events around the one call) | total.  rounds_needed: the fewest launches of the chunk hand-over after which the call
              reports no NOT_SYNCED (the call is run at rounds = 1, 2, ...); the timed calls use the default.
  uncrop      dataset.uncrop_faces end to end over 4 .jpg photos of 1600 x 2000 with 256 x 256 .jpg edits, jpeg='device', decode='host'
              and decode='device' alternating
The split of the call into its kernels comes from a kernel trace in a run of its own (--kernels-only under rocprofv3 --kernel-trace
--output-format csv): device events cannot be placed between launches that one C call enqueues.  --kernel-trace CSV adds that trace's
per-kernel times (the memsets are not kernels of the library and are left out) to an existing JSON.

    python tools/jpeg_decode_time.py [--repeats 20] [--out profiles/jpeg_decode.json] [--kernels-only] [--kernel-trace kernel_trace.csv]

--restart: the same four inputs written with restart_marker_rows=1 (a DRI segment and RST0..RST7, as cameras write them) ->
profiles/jpeg_decode_rst.json.  The yardstick is what the parent commit does for such files under --decode device: they are fallbacks,
so Pillow decode per file, np.stack, one upload of the pixels.  The device side is jpegdec.parse_jpeg_restart | upload | ch_jpeg_decode_rst.
Beside it, in the same loop, the same pixels without markers through ch_jpeg_decode (events around the call), and for both the fewest
launches of the chunk hand-over after which no stream is NOT_SYNCED.  --kernels-only and --kernel-trace work as above, four calls with
markers and then four without per shape.
"""
import argparse
import csv
import io
import json
import os
import re
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


def verdict(host, dev):
    return 'device faster' if dev['max_ms'] < host['min_ms'] else 'host faster' if dev['min_ms'] > host['max_ms'] else 'within the spread'


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


def restart_kernel_trace(args):
    with open(args.out) as f:
        out = json.load(f)
    with open(args.kernel_trace) as f:
        rows = sorted((r for r in csv.DictReader(f) if re.search(r'jpeg_\w+_kernel', r['Kernel_Name'])), key=lambda r: int(r['Start_Timestamp']))
    ks = [(re.search(r'jpeg_\w+_kernel', r['Kernel_Name']).group(0), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows]
    per_call = 8 + 5
    assert len(ks) == 8 * per_call * len(out['inputs']), len(ks)               # --restart --kernels-only: 4 + 4 calls per shape
    for i, row in enumerate(out['inputs']):
        for key, nth in (('kernel_us_restart', 3), ('kernel_us_plain', 7)):    # the last call of each kind
            call = ks[(8 * i + nth) * per_call:(8 * i + nth + 1) * per_call]
            assert [k for k, _ in call[8:]] == ['jpeg_chain_kernel', 'jpeg_write_kernel', 'jpeg_dc_kernel', 'jpeg_idct_kernel', 'jpeg_colour_kernel']
            row[key] = {'jpeg_sync_kernel_per_launch': [round(v, 1) for _, v in call[:8]], **{k: round(v, 1) for k, v in call[8:]}}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('added the kernel times to', args.out)


def restart_main(args):
    if args.kernel_trace:
        return restart_kernel_trace(args)
    import torch
    from PIL import Image
    from ctrlhair_amd import jpegdec, lib
    dev = torch.device('cuda', 0)
    dec = jpegdec.JpegDecoder(lib.Handle(0), dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sync = torch.cuda.synchronize

    def saved(px, **kw):
        buf = io.BytesIO()
        Image.fromarray(px).save(buf, 'JPEG', quality=90, **kw)
        return buf.getvalue()

    def rounds_needed(streams, tables, H, W, restart):
        return next(r for r in range(1, 65)
                    if jpegdec.NOT_SYNCED not in dec.decode_streams(streams, tables, H, W, 3, 2, rounds=r, restart=restart)[1].cpu().tolist())

    shapes = [('photo3000x4000', 3000, 4000, 1), ('photo1600x2000', 1600, 2000, 1), ('crop1024', 1024, 1024, 1), ('crop256x16', 256, 256, 16)]
    rows = []
    for name, H, W, N in shapes:
        px = [photo(H, W, seed=7 * k + H) for k in range(N)]
        blobs, plain = [saved(p, restart_marker_rows=1) for p in px], [saved(p) for p in px]
        parsed, pp = [jpegdec.parse_jpeg_restart(b) for b in blobs], [jpegdec.parse_jpeg(b) for b in plain]
        streams, tables, restart = [p[5] for p in parsed], [p[4] for p in parsed], [p[6] for p in parsed]
        pstreams, ptables = [p[5] for p in pp], [p[4] for p in pp]
        assert all(r == (W + 15) // 16 for r in restart)
        host_px = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert('RGB')) for b in blobs])
        for _ in range(4 if args.kernels_only else 1):
            img, status = dec.decode_streams(streams, tables, H, W, 3, 2, restart=restart)
        assert status.cpu().tolist() == [0] * N and np.array_equal(img.cpu().numpy(), host_px), name
        for _ in range(4 if args.kernels_only else 1):
            img, status = dec.decode_streams(pstreams, ptables, H, W, 3, 2)
        assert status.cpu().tolist() == [0] * N and np.array_equal(img.cpu().numpy(), host_px), name      # the same pixels without markers
        if args.kernels_only:
            continue
        t = {k: [] for k in ('host_total', 'host_decode', 'host_upload', 'dev_parse', 'dev_upload', 'dev_kernels', 'dev_total', 'plain_kernels')}
        for rep in range(-2, args.repeats):
            sync()
            t0 = time.perf_counter()
            hp = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert('RGB')) for b in blobs])
            t1 = time.perf_counter()
            up = torch.from_numpy(hp).to(dev)
            sync()
            t2 = time.perf_counter()
            ps = [jpegdec.parse_jpeg_restart(b) for b in blobs]
            t3 = time.perf_counter()
            e0, e1, e2, e3 = ev(), ev(), ev(), ev()
            uploaded = dec.upload([p[5] for p in ps], [p[4] for p in ps], [p[6] for p in ps])
            sync()
            t4 = time.perf_counter()
            e0.record()
            got, st = dec.launch(uploaded, H, W, 3, 2)
            e1.record()
            sync()
            t5 = time.perf_counter()
            uploaded = dec.upload(pstreams, ptables)
            sync()
            e2.record()
            got2, st2 = dec.launch(uploaded, H, W, 3, 2)
            e3.record()
            sync()
            if rep >= 0:
                for k, v in (('host_total', t2 - t0), ('host_decode', t1 - t0), ('host_upload', t2 - t1), ('dev_parse', t3 - t2), ('dev_upload', t4 - t3),
                             ('dev_total', t5 - t2)):
                    t[k].append(v * 1e3)
                t['dev_kernels'].append(e0.elapsed_time(e1))
                t['plain_kernels'].append(e2.elapsed_time(e3))
            del up, got, got2
        row = {'input': name, 'batch': N, 'H': H, 'W': W, 'quality': 90, 'sampling': '4:2:0', 'restart_interval_mcus': restart[0],
               'markers': sum(len(re.findall(rb'\xff[\xd0-\xd7]', s)) for s in streams), 'file_bytes': sum(map(len, blobs)),
               'scan_bytes': sum(map(len, streams)), 'plain_scan_bytes': sum(map(len, pstreams)), 'chunks': sum(-(-len(s) // 8192) for s in streams),
               'rounds_needed': rounds_needed(streams, tables, H, W, restart), 'plain_rounds_needed': rounds_needed(pstreams, ptables, H, W, None),
               'rounds_default': 8}
        row.update({k: spread(v) for k, v in t.items()})
        row['verdict'] = verdict(row['host_total'], row['dev_total'])
        row['gap_ms'] = round(row['host_total']['median_ms'] - row['dev_total']['median_ms'], 4)
        row['yardstick_spread_ms'] = round(row['host_total']['max_ms'] - row['host_total']['min_ms'], 4)
        row['gap_exceeds_yardstick_spread'] = abs(row['gap_ms']) > row['yardstick_spread_ms']
        row['kernels_restart_against_plain'] = verdict(row['plain_kernels'], row['dev_kernels']).replace('device', 'restart').replace('host', 'plain')
        row['fewer_launches_with_markers'] = row['rounds_needed'] < row['plain_rounds_needed']
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.kernels_only:
        return
    out = {'what': 'ch_jpeg_decode_rst over files written with restart_marker_rows=1 against what the parent commit does for them under '
                   '--decode device (Pillow decode per file + one upload of the pixels); beside it the same pixels without markers through '
                   'ch_jpeg_decode; median (min - max), all sides alternating in one loop; one session', 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'inputs': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--restart', action='store_true', help='the restart-interval measurement (see the module docstring) -> profiles/jpeg_decode_rst.json')
    ap.add_argument('--kernels-only', action='store_true', help='only the ch_jpeg_decode calls, 3 per shape (for a kernel trace)')
    ap.add_argument('--kernel-trace', default=None, help='the kernel trace (CSV) of a --kernels-only run under rocprofv3 --kernel-trace: its per-kernel times of the last call of every shape are added to the JSON at --out; nothing is run')
    ap.add_argument('--out', default=None, help='profiles/jpeg_decode.json, or profiles/jpeg_decode_rst.json with --restart')
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, 'profiles', 'jpeg_decode_rst.json' if args.restart else 'jpeg_decode.json')
    if args.restart:
        return restart_main(args)
    if args.kernel_trace:
        with open(args.out) as f:
            out = json.load(f)
        with open(args.kernel_trace) as f:
            ks = [(re.search(r'jpeg_\w+_kernel', r['Kernel_Name']).group(0), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                  for r in csv.DictReader(f) if re.search(r'jpeg_\w+_kernel', r['Kernel_Name'])]
        per_call = 8 + 5                                                       # the default's sync launches, then chain, write, dc, idct, colour
        assert len(ks) == 4 * per_call * len(out['inputs']), len(ks)           # --kernels-only: 4 calls per shape
        for i, row in enumerate(out['inputs']):
            call = ks[(4 * i + 3) * per_call:(4 * i + 4) * per_call]           # the last call of the shape
            assert [k for k, _ in call[8:]] == ['jpeg_chain_kernel', 'jpeg_write_kernel', 'jpeg_dc_kernel', 'jpeg_idct_kernel', 'jpeg_colour_kernel']
            row['kernel_us'] = {'jpeg_sync_kernel_per_launch': [round(v, 1) for _, v in call[:8]], **{k: round(v, 1) for k, v in call[8:]}}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
        print('added the kernel times to', args.out)
        return
    import torch
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import jpegdec, lib
    from ctrlhair_amd.alignment import FaceAligner
    import unalign_cases as UC
    dev = torch.device('cuda', 0)
    handle = lib.Handle(0)
    dec = jpegdec.JpegDecoder(handle, dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sync = torch.cuda.synchronize

    def saved(px):
        buf = io.BytesIO()
        Image.fromarray(px).save(buf, 'JPEG', quality=90)
        return buf.getvalue()

    shapes = [('photo3000x4000', 3000, 4000, 1), ('photo1600x2000', 1600, 2000, 1), ('crop1024', 1024, 1024, 1), ('crop256x16', 256, 256, 16)]
    rows = []
    for name, H, W, N in shapes:
        blobs = [saved(photo(H, W, seed=7 * k + H)) for k in range(N)]
        parsed = [jpegdec.parse_jpeg(b) for b in blobs]
        streams, tables = [p[5] for p in parsed], [p[4] for p in parsed]
        host_px = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert('RGB')) for b in blobs])
        img, status = dec.decode_streams(streams, tables, H, W, 3, 2)
        assert status.cpu().tolist() == [0] * N and np.array_equal(img.cpu().numpy(), host_px), name
        if args.kernels_only:
            for _ in range(3):
                dec.decode_streams(streams, tables, H, W, 3, 2)
            continue
        needed = next(r for r in range(1, 65) if jpegdec.NOT_SYNCED not in dec.decode_streams(streams, tables, H, W, 3, 2, rounds=r)[1].cpu().tolist())
        t = {k: [] for k in ('host_total', 'host_decode', 'host_upload', 'dev_parse', 'dev_upload', 'dev_kernels', 'dev_total')}
        for rep in range(-2, args.repeats):
            sync()
            t0 = time.perf_counter()
            px = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert('RGB')) for b in blobs])
            t1 = time.perf_counter()
            up = torch.from_numpy(px).to(dev)
            sync()
            t2 = time.perf_counter()
            ps = [jpegdec.parse_jpeg(b) for b in blobs]
            t3 = time.perf_counter()
            e0, e1 = ev(), ev()
            uploaded = dec.upload([p[5] for p in ps], [p[4] for p in ps])
            sync()
            t4 = time.perf_counter()
            e0.record()
            got, st = dec.launch(uploaded, H, W, 3, 2)
            e1.record()
            sync()
            t5 = time.perf_counter()
            if rep >= 0:
                for k, v in (('host_total', t2 - t0), ('host_decode', t1 - t0), ('host_upload', t2 - t1), ('dev_parse', t3 - t2), ('dev_upload', t4 - t3),
                             ('dev_total', t5 - t2)):
                    t[k].append(v * 1e3)
                t['dev_kernels'].append(e0.elapsed_time(e1))
            del up, got
        row = {'input': name, 'batch': N, 'H': H, 'W': W, 'quality': 90, 'sampling': '4:2:0', 'file_bytes': sum(map(len, blobs)),
               'scan_bytes': sum(map(len, streams)), 'chunks': sum(-(-len(s) // 8192) for s in streams), 'rounds_needed': needed,
               'rounds_default': 8}
        row.update({k: spread(v) for k, v in t.items()})
        row['verdict'] = verdict(row['host_total'], row['dev_total'])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.kernels_only:
        return

    # dataset uncrop end to end: the landmarks of a test case, scaled to photos of ten times its size
    tmp = tempfile.mkdtemp(prefix='jpeg_decode_time_')
    c = UC.inputs('a_magnify')
    scale = 10
    H, W = c['photo'].shape[0] * scale, c['photo'].shape[1] * scale
    names = [f'{i:03d}.jpg' for i in range(4)]
    photos, edits = os.path.join(tmp, 'photos'), os.path.join(tmp, 'edits')
    os.makedirs(photos)
    for i, n in enumerate(names):
        Image.fromarray(photo(H, W, seed=10 + i)).save(os.path.join(photos, n), quality=90)
    lms = {n: np.asarray(c['lm'], np.float64) * scale for n in names}
    aligner = FaceAligner(handle, dev)
    D.crop_faces(aligner, photos, edits, 'ds', lms, size=256)
    outd = {m: os.path.join(tmp, 'uncrop_' + m) for m in ('host', 'device')}
    acc = {m: [] for m in outd}
    stats = {}
    for rep in range(-1, args.repeats):
        for m in outd:
            sync()
            t0 = time.perf_counter()
            done, _ = D.uncrop_faces(aligner, photos, edits, outd[m], 'ds', lms, jpeg='device', decode=m, stats=stats)
            sync()
            if rep >= 0:
                acc[m].append((time.perf_counter() - t0) * 1e3 / len(names))
            assert len(done) == len(names) and stats['fallbacks'] == 0
    for n in names:
        with open(os.path.join(outd['host'], n), 'rb') as a, open(os.path.join(outd['device'], n), 'rb') as b:
            assert a.read() == b.read(), n
    uncrop = {'photos': len(names), 'H': H, 'W': W, 'edit_side': 256, 'jpeg': 'device', 'per_photo_decode_host': spread(acc['host']),
              'per_photo_decode_device': spread(acc['device']), 'files_equal': True}
    uncrop['verdict'] = verdict(uncrop['per_photo_decode_host'], uncrop['per_photo_decode_device'])
    print(json.dumps(uncrop), flush=True)
    out = {'what': 'ch_jpeg_decode (one upload of the compressed bytes, entropy decode parallel within each scan, IDCT, upsampling and colour on '
                   'the device) against Pillow decode per file + one upload of the pixels; median (min - max), the two sides alternating; one '
                   'session', 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'inputs': rows,
           'dataset_uncrop_end_to_end': uncrop}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
