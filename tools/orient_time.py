"""Times the EXIF orientation on the device against what one would write without it -> profiles/orient.json.  One session, after
warm-up calls of every side, median (min - max) of --repeats calls, the sides alternating in one loop whose order rotates.

  shapes      photo12mp   orientation 6 of a 3000 x 4000 RGB photo (stored H x W)
              photo3mp    orientation 6 of a 1600 x 2000 RGB photo
              batch16     16 RGB images of 256 x 256 with orientations 2..8 mixed
  sides       kernel      orient.Orienter.apply: ch_orient_u8, one launch per batch (wall clock with a synchronisation, and device events
                          around the call; the call includes the packing, the descriptors' upload and the allocation of the result)
              entry       the ch_orient_u8 call alone, on a batch packed and buffers allocated beforehand (descriptor upload + launch)
              torch       the yardstick: per image the torch expression of the orientation on the device, e.g.
                          t.transpose(0, 1).flip(1).contiguous() for 6 -- N generic strided byte copies
              host        download + Pillow's Image.transpose + upload
  beside that the kernel's bytes moved (each byte read once and written once) over the 6.29 TB/s copy rate of the README's other rows --
  repeated calls on the same photo sit partly in the 256 MiB Infinity Cache, so that share flatters the HBM figure --, the cost of
  photometa.read_metadata per file, and `dataset crop --decode device` per photo on four 1600 x 2000 .jpg photos: the parent commit's
  code path (no option, untagged upright files: the yardstick) against --orient on the same pictures stored turned with tag 6.
The results of the three sides are compared once per shape (equal bytes).  No ratio is fixed in advance: each row carries the gap between
the medians beside the yardstick's own spread (max - min).

    python tools/orient_time.py [--repeats 20] [--out profiles/orient.json] [--small]

--small: small shapes and few repeats, to try the tool out.
"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

COPY_RATE = 6.29e12          # bytes/s, the HBM copy rate the README's rows use


def spread(v, unit='ms'):
    v = sorted(v)
    return {f'median_{unit}': round(float(np.median(v)), 4), f'min_{unit}': round(v[0], 4), f'max_{unit}': round(v[-1], 4)}


def compare(yard, new, unit='ms'):
    """Less is better.  The verdict by the spreads, and the gap of the medians beside the yardstick's own spread."""
    y, d = [yard[f'{k}_{unit}'] for k in ('min', 'median', 'max')], [new[f'{k}_{unit}'] for k in ('min', 'median', 'max')]
    verdict = 'faster' if d[2] < y[0] else 'slower' if d[0] > y[2] else 'within the spread'
    gap, own = y[1] - d[1], y[2] - y[0]
    return {'verdict': verdict, f'gap_{unit}': round(gap, 4), f'yardstick_spread_{unit}': round(own, 4), 'gap_exceeds_yardstick_spread': abs(gap) > own,
            'median_below_yardstick_min': d[1] < y[0]}


def torch_expression(t, o):
    """The upright image of a [H,W,C] device tensor as one would write it in torch."""
    if o == 2:
        return t.flip(1).contiguous()
    if o == 3:
        return t.flip(0, 1).contiguous()
    if o == 4:
        return t.flip(0).contiguous()
    u = t.transpose(0, 1)
    return {5: u, 6: u.flip(1), 7: u.flip(0, 1), 8: u.flip(0)}[o].contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'orient.json'))
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    from PIL import Image
    from jpeg_decode_time import photo
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import lib, orient as O, photometa
    from ctrlhair_amd.alignment import FaceAligner
    from tests import align_oracle as AO
    sync = torch.cuda.synchronize
    dev = torch.device('cuda', 0)
    handle = lib.Handle(0)
    orienter = O.Orienter(handle, dev)
    repeats = min(args.repeats, 3) if args.small else args.repeats
    pillow = {2: Image.Transpose.FLIP_LEFT_RIGHT, 3: Image.Transpose.ROTATE_180, 4: Image.Transpose.FLIP_TOP_BOTTOM, 5: Image.Transpose.TRANSPOSE,
              6: Image.Transpose.ROTATE_270, 7: Image.Transpose.TRANSVERSE, 8: Image.Transpose.ROTATE_90}
    out = {'what': 'EXIF orientation of uint8 RGB images on the device: Orienter.apply (ch_orient_u8, one launch per batch) against the torch '
                   'expression per image (the yardstick) and against download + Pillow transpose + upload; ms per call, median (min - max), the '
                   'sides alternating in one loop; one session', 'repeats': repeats, 'device': torch.cuda.get_device_name(0),
           'copy_rate_bytes_per_s': COPY_RATE, 'shapes': [], 'read_metadata': [], 'crop_job': None}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)

    big, mid = ((3000, 4000), (1600, 2000)) if not args.small else ((300, 400), (160, 200))
    specs = [('photo12mp', [photo(*big, seed=1)], [6]), ('photo3mp', [photo(*mid, seed=2)], [6]),
             ('batch16', [photo(256, 256, seed=10 + k) for k in range(16)], [2 + k % 7 for k in range(16)])]
    for name, host_px, orients in specs:
        dev_px = [torch.from_numpy(a).to(dev) for a in host_px]
        nbytes = 2 * sum(a.size for a in host_px)

        def kernel():
            return orienter.apply(dev_px, orients)

        def expression():
            return [torch_expression(t, o) for t, o in zip(dev_px, orients)]

        def host():
            return [torch.from_numpy(np.asarray(Image.fromarray(t.cpu().numpy()).transpose(pillow[o]))).to(dev) for t, o in zip(dev_px, orients)]

        # the entry point alone, on a batch packed and buffers allocated beforehand: what Orienter.apply spends outside it is host work
        import ctypes
        blob, _, total = O.pack_batch([t.data_ptr() for t in dev_px], [tuple(t.shape) for t in dev_px], orients)
        blob = np.ascontiguousarray(blob)
        dst, ws = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(65536, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def entry():
            handle.call('ch_orient_u8', blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, len(dev_px), dst.data_ptr(), total, ws.data_ptr(),
                        ws.numel(), stream)

        sides = (('kernel', kernel), ('entry', entry), ('torch', expression), ('host', host))
        results = {k: f() for k, f in sides if k != 'entry'}
        entry()
        sync()
        assert torch.equal(dst, torch.cat([r.reshape(-1) for r in results['kernel']])), name      # (256-aligned offsets of 256-multiples: tight)
        for n, a in enumerate(host_px):
            want = torch.from_numpy(np.ascontiguousarray(O.orient_numpy(a, orients[n])))
            assert all(torch.equal(results[k][n].cpu(), want) for k in results), (name, n)
        del results
        t = {k: [] for k, _ in sides}
        ev = {k: [] for k, _ in sides if k != 'host'}
        for rep in range(-3, repeats):
            for k, f in sides[rep % 4:] + sides[:rep % 4]:             # the order rotates: no side always runs behind the same other one
                sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                r = f()
                e1.record()
                sync()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 0:
                    t[k].append(dt)
                    if k in ev:
                        ev[k].append(e0.elapsed_time(e1))
                del r
        row = {'shape': name, 'N': len(host_px), 'H': host_px[0].shape[0], 'W': host_px[0].shape[1], 'orientations': orients,
               'bytes_moved': nbytes, 'kernel': spread(t['kernel']), 'kernel_events': spread(ev['kernel']), 'torch': spread(t['torch']),
               'torch_events': spread(ev['torch']), 'host': spread(t['host'])}
        row['kernel_vs_torch'] = compare(row['torch'], row['kernel'])
        row['kernel_vs_torch_events'] = compare(row['torch_events'], row['kernel_events'])
        row['kernel_vs_host'] = compare(row['host'], row['kernel'])
        row['entry'] = spread(t['entry'])
        row['entry_events'] = spread(ev['entry'])
        row['entry_vs_torch_events'] = compare(row['torch_events'], row['entry_events'])
        rate = nbytes / (row['entry_events']['median_ms'] * 1e-3)
        row['entry_bytes_per_s_by_events'] = rate
        row['share_of_copy_rate'] = round(rate / COPY_RATE, 4)
        row['note'] = ('kernel / kernel_events span the whole Orienter.apply call (packing, allocation, descriptor upload, one launch), entry_events '
                       'the ch_orient_u8 call alone on a batch packed and buffers allocated beforehand (descriptor upload and launch), timed in the '
                       'same rotating loop as the other sides; repeated calls on the same ' +
                       f'{nbytes / 1e6:.0f} MB sit partly in the 256 MiB Infinity Cache, so the share flatters the HBM figure')
        out['shapes'].append(row)
        print(json.dumps(row), flush=True)
        flush()
        del dev_px

    # read_metadata per file: a camera-like JPEG with EXIF and a profile, a plain JPEG, a PNG with eXIf
    exif = Image.Exif()
    exif[0x0112], exif[0x010F], exif[0x0132] = 6, 'a camera maker', '2024:05:06 07:08:09'
    icc = np.random.default_rng(5).integers(0, 256, 540000 if not args.small else 3000, dtype=np.uint8).tobytes()
    files = {}
    for label, fmt, kw in (('jpeg 1600x2000, EXIF + 540 kB profile', 'JPEG', dict(exif=exif, icc_profile=icc, quality=90)),
                           ('jpeg 1600x2000, no metadata', 'JPEG', dict(quality=90)), ('png 256x256, eXIf', 'PNG', dict(exif=exif))):
        buf = io.BytesIO()
        Image.fromarray(photo(*(mid if fmt == 'JPEG' else (256, 256)), seed=3)).save(buf, fmt, **kw)
        files[label] = buf.getvalue()
    for label, data in files.items():
        v = []
        for rep in range(-3, max(repeats, 20)):
            t0 = time.perf_counter()
            m = photometa.read_metadata(data)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 0:
                v.append(dt)
        row = {'file': label, 'file_bytes': len(data), 'orientation': m[0], 'read_metadata': spread(v)}
        out['read_metadata'].append(row)
        print(json.dumps(row), flush=True)
    flush()

    # dataset crop --decode device per photo: the parent's code path on untagged upright files against --orient on the turned, tagged ones
    tmp = tempfile.mkdtemp(prefix='orient_time_')
    try:
        aligner = FaceAligner(handle, dev)
        Hs, Ws = mid                                                     # stored landscape ...
        plain, tagged = os.path.join(tmp, 'plain'), os.path.join(tmp, 'tagged')
        os.makedirs(plain), os.makedirs(tagged)
        lms = {}
        for k in range(4):
            up = photo(Ws, Hs, seed=40 + k)                              # ... upright portrait
            n = f'p{k}.jpg'
            Image.fromarray(up).save(os.path.join(plain, n), quality=90)
            stored = np.ascontiguousarray(O.orient_numpy(up, O.inverse_orientation(6)))
            assert stored.shape[:2] == (Hs, Ws)
            tag = Image.Exif()
            tag[0x0112] = 6
            Image.fromarray(stored).save(os.path.join(tagged, n), quality=90, exif=tag)
            lms[n] = AO.make_landmarks(100 + k, (Hs * 0.5, Ws * 0.45), Hs * 0.09, 5.0)
        jobs = (('parent_path_untagged', plain, {}), ('orient_tagged', tagged, {'orient': True}))
        t = {k: [] for k, _, _ in jobs}
        for rep in range(-2, repeats):
            for k, src, kw in jobs:
                stats = {}
                sync()
                t0 = time.perf_counter()
                done, _ = D.crop_faces(aligner, src, os.path.join(tmp, 'out_' + k), 'ds', lms, size=256, decode='device', jpeg='device', stats=stats, **kw)
                sync()
                dt = (time.perf_counter() - t0) * 1e3 / 4
                assert len(done) == 4 and stats['fallbacks'] == 0
                if rep >= 0:
                    t[k].append(dt)
        row = {'what': 'dataset crop --decode device --jpeg device, ms per photo, four 1600 x 2000 .jpg photos at quality 90, 256 px crops; the '
                       'yardstick is the call without the option on untagged upright files (the parent commit\'s code path), the other side --orient '
                       'on the same pictures stored turned with tag 6 (other DCT blocks, so the crops differ slightly)',
               'parent_path_untagged': spread(t['parent_path_untagged']), 'orient_tagged': spread(t['orient_tagged'])}
        row['orient_vs_parent_path'] = compare(row['parent_path_untagged'], row['orient_tagged'])
        out['crop_job'] = row
        print(json.dumps(row), flush=True)
        flush()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
