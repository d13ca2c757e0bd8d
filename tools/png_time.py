"""Times the device PNG encoder against the path it replaces -> profiles/png_encode.json.  One session, after warm-up, median (min - max)
of --repeats runs, for
    the two direction-search sheets (1792 x 2560 texture, 1792 x 5120 shape, RGB; made as tools/direction_time.py makes them: procedural
    ngf = 64 weights, 10 images x 6 values at 256 x 256), 16 label maps of 256 x 256 (L, one batched call), a 3000 x 4000 RGB photo:
  yardstick   the download of the uint8 array (hostutil.to_host) + Image.fromarray(...).save at Pillow's default level (6); level 1 as well
  device      ch_png_encode (filter + deflate + gather, device events around the one call), the two downloads (lengths, compressed
              bytes), CRC + container (pngenc.wrap_png), and the file write; file sizes beside Pillow's at levels 6 and 1
  per candidate of a direction search: sweep + sheet + statistics, then the sheet written by either path (find_directions png='host' |
              'device'), the two alternating in the same loop
The split of the call into its three kernels comes from a kernel trace in a run of its own (--kernels-only under rocprofv3
--kernel-trace --stats): device events cannot be placed between launches that one C call enqueues.

    python tools/png_time.py [--repeats 20] [--out profiles/png_encode.json] [--kernels-only]
"""
import argparse
import io
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--candidates', type=int, default=2)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--kernels-only', action='store_true', help='only the ch_png_encode calls (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode.json'))
    args = ap.parse_args()
    import torch
    from PIL import Image
    import png_oracle as PO
    from ctrlhair_amd import directions as DS
    from ctrlhair_amd import hostutil as U
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import procedural_weights
    from ctrlhair_amd.pipeline import EditPipeline
    from ctrlhair_amd.pngenc import PngEncoder, wrap_png
    sync = torch.cuda.synchronize
    S, I, V = 256, 10, 6
    values = np.linspace(-2.5, 2.5, V)
    pipe = EditPipeline(procedural_weights(0, args.ngf), device=0, img_size=S, max_batch=20)
    search = DS.DirectionSearch(pipe, torch.from_numpy(P.synthetic_images(I, S, seed=3)).cuda())
    enc = PngEncoder(search.handle, search.device)
    shapes = []
    for att in ('texture', 'shape'):
        images, masks = search.sweep(att, DS.candidate_direction(DS.DIMS[att], [], 0, 0), values)
        shapes.append((f'{att} sheet', search.sheet(att, images, masks).canvas[None].clone()))
    shapes.append(('16 label maps', torch.from_numpy(np.stack([PO.label_map(256, seed=s) for s in range(16)])).cuda()))
    shapes.append(('photo', torch.from_numpy(photo(3000, 4000)[None]).cuda()))
    tmp = tempfile.mkdtemp()
    rows = []
    for name, x in shapes:
        N, H, W = (int(v) for v in x.shape[:3])
        C = int(x.shape[3]) if x.dim() == 4 else 1
        row = {'input': name, 'N': N, 'H': H, 'W': W, 'C': C, 'pixel_bytes': N * H * W * C}
        paths = [os.path.join(tmp, f'{n}.png') for n in range(N)]
        enc.streams(x)                                                            # warm-up: code objects, workspace, pinned buffer
        sync()
        t = {k: [] for k in ('kernels_event', 'download', 'crc_wrap', 'write', 'total')}
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            streams = enc.streams(x)                                              # kernels + both downloads (synchronises)
            t1 = time.perf_counter()
            files = [wrap_png(z, H, W, C) for z in streams]
            t2 = time.perf_counter()
            for p, f in zip(paths, files):
                with open(p, 'wb') as fh:
                    fh.write(f)
            t3 = time.perf_counter()
            # the kernels alone: the same call again between two events, nothing downloaded
            ws, out = enc._ws, enc._out
            sizes = torch.empty(N, dtype=torch.int64, device='cuda')
            bound = int(enc.handle.lib.ch_png_zlib_bound(H, W, C))
            e0.record()
            enc.handle.call('ch_png_encode', x.data_ptr(), N, H, W, C, -1, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(), ws.numel(),
                            torch.cuda.current_stream().cuda_stream)
            e1.record()
            e1.synchronize()
            k_ms = e0.elapsed_time(e1)
            assert bound >= max(len(z) for z in streams)
            t['kernels_event'].append(k_ms)
            t['download'].append((t1 - t0) * 1e3 - k_ms)                          # the call's host time minus its kernels
            t['crc_wrap'].append((t2 - t1) * 1e3)
            t['write'].append((t3 - t2) * 1e3)
            t['total'].append((t3 - t0) * 1e3)
        row['device'] = {k: spread(v) for k, v in t.items()}
        row['device_file_bytes'] = sum(len(f) for f in files)
        if not args.kernels_only:
            for level, key in ((None, 'pillow_default'), (1, 'pillow_level1')):
                kw = {} if level is None else {'compress_level': level}
                ms, parts = [], {'download': [], 'encode': [], 'write': []}
                for _ in range(args.repeats if level is None else max(3, args.repeats // 4)):
                    sync()
                    t0 = time.perf_counter()
                    arr = U.to_host(x)
                    t1 = time.perf_counter()
                    blobs = []
                    for n in range(N):
                        b = io.BytesIO()
                        Image.fromarray(arr[n]).save(b, format='PNG', **kw)
                        blobs.append(b.getvalue())
                    t2 = time.perf_counter()
                    for p, f in zip(paths, blobs):
                        with open(p, 'wb') as fh:
                            fh.write(f)
                    t3 = time.perf_counter()
                    ms.append((t3 - t0) * 1e3)
                    for k, a, b in (('download', t0, t1), ('encode', t1, t2), ('write', t2, t3)):
                        parts[k].append((b - a) * 1e3)
                row[key] = {'total': spread(ms), **{k: spread(v) for k, v in parts.items()}, 'file_bytes': sum(len(b) for b in blobs)}
                for n in range(N):                                                # the same pixels
                    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[n]))), np.asarray(Image.open(io.BytesIO(blobs[n]))))
            y, d = row['pillow_default']['total'], row['device']['total']
            row['gap_ms'] = round(y['median_ms'] - d['median_ms'], 4)
            row['yardstick_spread_ms'] = round(y['max_ms'] - y['min_ms'], 4)
            row['gain_exceeds_yardstick_spread'] = bool(row['gap_ms'] > row['yardstick_spread_ms'])
        rows.append(row)
        print(json.dumps(row), flush=True)

    per_candidate = {}
    if not args.kernels_only:
        K = args.candidates
        for att in ('texture', 'shape'):
            cands = [DS.candidate_direction(DS.DIMS[att], [], 0, k) for k in range(K)]
            path = os.path.join(tmp, 'sheet.png')
            acc = {'host': [], 'device': []}

            def candidate(d, mode):
                sync()
                t0 = time.perf_counter()
                images, masks = search.sweep(att, d, values)
                sheet = search.sheet(att, images, masks)
                DS.score(att, search.stats(images, masks), values, S, S)
                if mode == 'host':
                    DS.write_png(path, sheet.numpy())
                else:
                    enc.write([path], sheet.canvas[None])
                sync()
                return (time.perf_counter() - t0) * 1e3
            for mode in acc:
                candidate(cands[0], mode)
            for _ in range(args.repeats):
                for mode in acc:                                                  # alternating in one loop
                    acc[mode].append(sum(candidate(d, mode) for d in cands) / K)
            per_candidate[att] = {m: spread(v) for m, v in acc.items()}
            print(att, per_candidate[att], flush=True)

    out = {'what': 'PNG files from device pixels: download + Pillow (yardstick, the path before the device encoder) against ch_png_encode + '
                   'download of the compressed bytes + CRC / container on the host; one session',
           'repeats': args.repeats, 'chunk_bytes': enc.chunk, 'device': torch.cuda.get_device_name(0), 'inputs': rows,
           'direction_search_per_candidate_with_sheet': per_candidate}
    if not args.kernels_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
