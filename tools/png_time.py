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

--stride: the distance mode (ch_png_encode_dist) -> profiles/png_encode_dist.json instead.  The two sheets with distances=() and with the
sheet's column pitch (ContactSheet.png_distances), the two alternating in one loop: total, kernels by events, CRC + container, stream
bytes beside Pillow's file; which share of the stream's bytes and tokens went to the stride (from the rule, tests/png_dist_oracle.py);
per candidate of a direction search host | device | device with the stride.  --parent-lib PATH adds ch_png_encode (no distances) of this
build against another build of the library (the parent commit's), the two alternating, on all four inputs.

    python tools/png_time.py --stride [--parent-lib /path/to/libctrlhair_hip.so] [--repeats 20] [--out profiles/png_encode_dist.json]
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


def kernels_ms(lib, h, x, dist, enc):
    """One ch_png_encode (dist empty) or ch_png_encode_dist call of library `lib` on handle `h` between two device events: its three
    kernels, nothing downloaded."""
    import ctypes
    import torch
    N, H, W = (int(v) for v in x.shape[:3])
    C = int(x.shape[3]) if x.dim() == 4 else 1
    sizes = torch.empty(N, dtype=torch.int64, device='cuda')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream().cuda_stream
    tail = (enc._out.data_ptr(), sizes.data_ptr(), enc._ws.data_ptr(), enc._ws.numel(), stream)
    e0.record()
    if dist:
        rc = lib.ch_png_encode_dist(h, x.data_ptr(), N, H, W, C, -1, (ctypes.c_int * len(dist))(*dist), len(dist), *tail)
    else:
        rc = lib.ch_png_encode(h, x.data_ptr(), N, H, W, C, -1, *tail)
    e1.record()
    e1.synchronize()
    assert rc == 0, rc
    return e0.elapsed_time(e1)


def stride_shares(stream, chunk, dist):
    """Which share of the filtered bytes the rule gives to distance 1, to the stride and to literals (every chunk), and which share of
    the tokens are stride matches (every 16th chunk: the token walk is plain Python)."""
    import zlib
    import png_dist_oracle as DO
    data = zlib.decompress(stream)
    count, tokens, stride_tokens = np.zeros(3, np.int64), 0, 0
    for k, a in enumerate(range(0, len(data), chunk)):
        part = data[a:a + chunk]
        cls = DO.classes(part, dist)
        count += [int((cls == 0).sum()), int((cls == 1).sum()), int((cls < 0).sum())]
        if k % 16 == 0:
            tk = DO.parse(part, dist)
            tokens += len(tk)
            stride_tokens += sum(1 for t in tk if t[0] == 'M' and t[2] == dist[0])
    return {'bytes_distance_1': round(count[0] / len(data), 4), 'bytes_stride': round(count[1] / len(data), 4),
            'bytes_literal': round(count[2] / len(data), 4), 'tokens_stride_of_sampled': round(stride_tokens / max(tokens, 1), 4),
            'tokens_sampled': tokens}


def stride_mode(args, search, enc, shapes, pitch, values, S, tmp):
    import ctypes
    import torch
    from PIL import Image
    from ctrlhair_amd import directions as DS
    from ctrlhair_amd import lib as L
    from ctrlhair_amd.pngenc import wrap_png
    sync = torch.cuda.synchronize
    lib, h = search.handle.lib, search.handle._h
    rows = []
    for name, x in shapes[:2]:
        N, H, W, C = (int(v) for v in x.shape)
        modes = {'()': (), 'stride': pitch[name]}
        row = {'input': name, 'H': H, 'W': W, 'C': C, 'pixel_bytes': H * W * C, 'stride_bytes': list(pitch[name])}
        path = os.path.join(tmp, 'sheet.png')
        t = {m: {k: [] for k in ('kernels_event', 'download', 'crc_wrap', 'write', 'total')} for m in modes}
        streams = {}
        for m, D in modes.items():
            enc.streams(x, distances=D)                                           # warm-up
        for _ in range(args.repeats):
            for m, D in modes.items():                                            # alternating in one loop
                sync()
                t0 = time.perf_counter()
                streams[m] = enc.streams(x, distances=D)[0]
                t1 = time.perf_counter()
                png = wrap_png(streams[m], H, W, C)
                t2 = time.perf_counter()
                with open(path, 'wb') as fh:
                    fh.write(png)
                t3 = time.perf_counter()
                k_ms = kernels_ms(lib, h, x, D, enc)
                for k, v in (('kernels_event', k_ms), ('download', (t1 - t0) * 1e3 - k_ms), ('crc_wrap', (t2 - t1) * 1e3),
                             ('write', (t3 - t2) * 1e3), ('total', (t3 - t0) * 1e3)):
                    t[m][k].append(v)
        for m in modes:
            row[m] = {**{k: spread(v) for k, v in t[m].items()}, 'stream_bytes': len(streams[m])}
        b = io.BytesIO()
        Image.fromarray(x[0].cpu().numpy()).save(b, format='PNG')
        row['pillow_default_file_bytes'] = len(b.getvalue())
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(wrap_png(streams['stride'], H, W, C)))), np.asarray(Image.open(b)))
        row['rule'] = stride_shares(streams['stride'], enc.chunk, pitch[name])
        rows.append(row)
        print(json.dumps(row), flush=True)

    per_candidate = {}
    K = args.candidates
    for att in ('texture', 'shape'):
        cands = [DS.candidate_direction(DS.DIMS[att], [], 0, k) for k in range(K)]
        path = os.path.join(tmp, 'sheet.png')
        acc = {'host': [], 'device': [], 'device_stride': []}

        def candidate(d, mode):
            sync()
            t0 = time.perf_counter()
            images, masks = search.sweep(att, d, values)
            sheet = search.sheet(att, images, masks)
            DS.score(att, search.stats(images, masks), values, S, S)
            if mode == 'host':
                DS.write_png(path, sheet.numpy())
            else:
                enc.write([path], sheet.canvas[None], distances=sheet.png_distances() if mode == 'device_stride' else ())
            sync()
            return (time.perf_counter() - t0) * 1e3
        for mode in acc:
            candidate(cands[0], mode)
        for _ in range(args.repeats):
            for mode in acc:
                acc[mode].append(sum(candidate(d, mode) for d in cands) / K)
        per_candidate[att] = {m: spread(v) for m, v in acc.items()}
        print(att, per_candidate[att], flush=True)

    against_parent = []
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for fn in ('ch_create', 'ch_destroy', 'ch_png_encode'):
            getattr(parent, fn).restype, getattr(parent, fn).argtypes = L.SYMBOLS[fn]
        ph = ctypes.c_void_p()
        assert parent.ch_create(0, ctypes.byref(ph)) == 0
        for name, x in shapes:
            enc.streams(x)                                                        # sizes the workspace for this input
            both = {'this': (lib, h), 'parent': (parent, ph)}
            acc = {k: [] for k in both}
            for k, (l, hh) in both.items():
                kernels_ms(l, hh, x, (), enc)
            for _ in range(args.repeats):
                for k, (l, hh) in both.items():
                    acc[k].append(kernels_ms(l, hh, x, (), enc))
            r = {'input': name, **{k: spread(v) for k, v in acc.items()}}
            r['this_median_within_parent_spread'] = bool(r['parent']['min_ms'] <= r['this']['median_ms'] <= r['parent']['max_ms']
                                                         or r['this']['median_ms'] <= r['parent']['median_ms'])
            against_parent.append(r)
            print(json.dumps(r), flush=True)
        parent.ch_destroy(ph)

    out = {'what': 'ch_png_encode_dist: contact sheets encoded with distances=() and with their column pitch; one session',
           'repeats': args.repeats, 'chunk_bytes': enc.chunk, 'device': torch.cuda.get_device_name(0), 'sheets': rows,
           'direction_search_per_candidate_with_sheet': per_candidate, 'ch_png_encode_against_parent_build_kernels_event': against_parent}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--candidates', type=int, default=2)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--kernels-only', action='store_true', help='only the ch_png_encode calls (for a kernel trace)')
    ap.add_argument('--stride', action='store_true', help='the distance mode: sheets with and without their column pitch -> png_encode_dist.json')
    ap.add_argument('--parent-lib', default=None, help='with --stride: another build of the library to time ch_png_encode against')
    ap.add_argument('--out', default=None, help='default: profiles/png_encode.json, with --stride profiles/png_encode_dist.json')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'png_encode_dist.json' if args.stride else 'png_encode.json')
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
    shapes, pitch = [], {}
    for att in ('texture', 'shape'):
        images, masks = search.sweep(att, DS.candidate_direction(DS.DIMS[att], [], 0, 0), values)
        sheet = search.sheet(att, images, masks)
        shapes.append((f'{att} sheet', sheet.canvas[None].clone()))
        pitch[f'{att} sheet'] = sheet.png_distances()
    shapes.append(('16 label maps', torch.from_numpy(np.stack([PO.label_map(256, seed=s) for s in range(16)])).cuda()))
    shapes.append(('photo', torch.from_numpy(photo(3000, 4000)[None]).cuda()))
    tmp = tempfile.mkdtemp()
    if args.stride:
        return stride_mode(args, search, enc, shapes, pitch, values, S, tmp)
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
