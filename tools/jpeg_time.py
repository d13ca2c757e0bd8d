"""Times the device JPEG encoder against the path it replaces -> profiles/jpeg_encode.json.  One session, after warm-up, median (min - max)
of --repeats runs, the two sides alternating in the same loop, for a photo-like 3000 x 4000 RGB image, 16 crops of 256 x 256 (one batched
call) and one 1024 x 1024 crop, at Pillow's defaults (quality 75, 4:2:0):
  yardstick   the download of the uint8 array (hostutil.to_host) + Image.fromarray(...).save(format='JPEG') at the same quality and
              subsampling + the file write.  Never the code under test.
  device      ch_jpeg_encode (its seven kernels, device events around the one call), the two downloads (lengths, compressed bytes), the
              container (jpegenc.wrap_jpeg), and the file write.  The files are compared with the yardstick's: they must be equal.
  uncrop      `dataset uncrop` end to end (dataset.uncrop_faces) over --photos .jpg photos of 1600 x 2000 with 256 x 256 edits,
              jpeg='host' against jpeg='device', alternating; the output folders are compared byte for byte.

    python tools/jpeg_time.py [--repeats 20] [--photos 4] [--out profiles/jpeg_encode.json]
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

QUALITY, SUBSAMPLING = 75, 2


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


def write_all(paths, blobs):
    for p, b in zip(paths, blobs):
        with open(p, 'wb') as fh:
            fh.write(b)


def folder_bytes(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--photos', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode.json'))
    args = ap.parse_args()
    import torch
    from PIL import Image
    import unalign_cases as UC
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import hostutil as U
    from ctrlhair_amd import lib as L
    from ctrlhair_amd.alignment import FaceAligner
    from ctrlhair_amd.jpegenc import JpegEncoder, wrap_jpeg
    sync = torch.cuda.synchronize
    handle = L.Handle(0)
    enc = JpegEncoder(handle, 'cuda:0')
    big = photo(3000, 4000)
    shapes = [('photo 3000 x 4000', big[None]), ('16 crops of 256 x 256', np.stack([photo(256, 256, seed=s) for s in range(16)])),
              ('crop 1024 x 1024', big[None, 900:1924, 1400:2424])]
    tmp = tempfile.mkdtemp()
    rows = []
    for name, arr in shapes:
        x = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        N, H, W, C = (int(v) for v in x.shape)
        row = {'input': name, 'N': N, 'H': H, 'W': W, 'C': C, 'pixel_bytes': N * H * W * C}
        paths = [os.path.join(tmp, f'{n}.jpg') for n in range(N)]
        enc.scans(x, QUALITY, SUBSAMPLING)                                        # warm-up: code objects, workspace, pinned buffer
        sync()
        dev = {k: [] for k in ('kernels_event', 'download', 'container', 'write', 'total')}
        yard = {k: [] for k in ('download', 'encode', 'write', 'total')}
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            scans = enc.scans(x, QUALITY, SUBSAMPLING)                            # kernels + both downloads (synchronises)
            t1 = time.perf_counter()
            files = [wrap_jpeg(s, H, W, C, QUALITY, SUBSAMPLING) for s in scans]
            t2 = time.perf_counter()
            write_all(paths, files)
            t3 = time.perf_counter()
            # the kernels alone: the same call again between two device events, nothing downloaded
            sizes = torch.empty(N, dtype=torch.int64, device='cuda')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            handle.call('ch_jpeg_encode', x.data_ptr(), N, H, W, C, QUALITY, SUBSAMPLING, enc._out.data_ptr(), sizes.data_ptr(),
                        enc._ws.data_ptr(), enc._ws.numel(), torch.cuda.current_stream().cuda_stream)
            e1.record()
            e1.synchronize()
            k_ms = e0.elapsed_time(e1)
            for k, v in (('kernels_event', k_ms), ('download', (t1 - t0) * 1e3 - k_ms), ('container', (t2 - t1) * 1e3),
                         ('write', (t3 - t2) * 1e3), ('total', (t3 - t0) * 1e3)):
                dev[k].append(v)
            sync()
            t0 = time.perf_counter()
            host = U.to_host(x)
            t1 = time.perf_counter()
            blobs = []
            for n in range(N):
                b = io.BytesIO()
                Image.fromarray(host[n]).save(b, format='JPEG', quality=QUALITY, subsampling=SUBSAMPLING)
                blobs.append(b.getvalue())
            t2 = time.perf_counter()
            write_all(paths, blobs)
            t3 = time.perf_counter()
            for k, a, b in (('download', t0, t1), ('encode', t1, t2), ('write', t2, t3), ('total', t0, t3)):
                yard[k].append((b - a) * 1e3)
        row['device'] = {k: spread(v) for k, v in dev.items()}
        row['yardstick_download_pillow'] = {k: spread(v) for k, v in yard.items()}
        row['file_bytes'] = sum(len(f) for f in files)
        row['files_equal_pillows'] = bool(files == blobs)
        y, d = row['yardstick_download_pillow']['total'], row['device']['total']
        row['gap_ms'] = round(y['median_ms'] - d['median_ms'], 4)
        row['yardstick_spread_ms'] = round(y['max_ms'] - y['min_ms'], 4)
        row['gain_exceeds_yardstick_spread'] = bool(row['gap_ms'] > row['yardstick_spread_ms'])
        rows.append(row)
        print(json.dumps(row), flush=True)

    # dataset uncrop end to end: the landmarks of a test case, scaled to photos of ten times its size
    c = UC.inputs('a_magnify')
    scale = 10
    H, W = c['photo'].shape[0] * scale, c['photo'].shape[1] * scale
    names = [f'{i:03d}.jpg' for i in range(args.photos)]
    photos, edits = os.path.join(tmp, 'photos'), os.path.join(tmp, 'edits')
    os.makedirs(photos)
    for i, n in enumerate(names):
        Image.fromarray(photo(H, W, seed=10 + i)).save(os.path.join(photos, n), quality=90)
    lms = {n: np.asarray(c['lm'], np.float64) * scale for n in names}
    aligner = FaceAligner(handle, torch.device('cuda', 0))
    D.crop_faces(aligner, photos, edits, 'ds', lms, size=256)
    out = {m: os.path.join(tmp, 'uncrop_' + m) for m in ('host', 'device')}
    acc = {m: [] for m in out}
    for m in out:
        D.uncrop_faces(aligner, photos, edits, out[m], 'ds', lms, jpeg=m)         # warm-up
    for _ in range(args.repeats):
        for m in out:
            sync()
            t0 = time.perf_counter()
            done, _ = D.uncrop_faces(aligner, photos, edits, out[m], 'ds', lms, jpeg=m)
            sync()
            acc[m].append((time.perf_counter() - t0) * 1e3 / len(done))
    uncrop = {'photos': len(names), 'H': H, 'W': W, 'edit_side': 256, 'per_photo': {m: spread(v) for m, v in acc.items()},
              'folders_equal': bool(folder_bytes(out['host']) == folder_bytes(out['device']))}
    y, d = uncrop['per_photo']['host'], uncrop['per_photo']['device']
    uncrop['gap_ms'] = round(y['median_ms'] - d['median_ms'], 4)
    uncrop['yardstick_spread_ms'] = round(y['max_ms'] - y['min_ms'], 4)
    uncrop['gain_exceeds_yardstick_spread'] = bool(uncrop['gap_ms'] > uncrop['yardstick_spread_ms'])
    print(json.dumps(uncrop), flush=True)

    result = {'what': 'JPEG files from device pixels: download + Pillow (yardstick, the path before the device encoder) against ch_jpeg_encode + '
                      'download of the compressed bytes + container on the host; one session, the two alternating',
              'quality': QUALITY, 'subsampling': '4:2:0', 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0), 'inputs': rows,
              'dataset_uncrop_end_to_end': uncrop}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
