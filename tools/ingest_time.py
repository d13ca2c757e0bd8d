"""Times the masks and codes jobs end to end with --decode host and --decode device -> profiles/ingest.json.  One session, after a
warm-up run of each side, median (min - max) of --repeats runs, the two sides alternating in one loop.

  directories jpeg1024   256 JPEG crops of 1024 x 1024 (quality 90, 4:2:0)
              png256     256 PNG crops of 256 x 256
              photo12mp  16 JPEG photos of 3000 x 4000 (masks only: the codes job reads aligned crops)
              photo-like procedural content (tools/jpeg_decode_time.py photo()), written by Pillow
  jobs        dataset.extract_masks and dataset.encode_sean_codes as `python -m ctrlhair_amd.dataset masks|codes --weights procedural
              --batch 16` runs them (full-size procedural networks, img_size 256, png='host'), in images per second
  yardstick   decode='host': what the parent commit does -- Pillow decode, Pillow / numpy resize and normalisation per image on one
              core, upload of float32
  device      decode='device': file bytes up, ch_jpeg_decode / ch_png_decode, one ch_ingest_images (and ch_ingest_labels) per batch
  ingest      beside that, one batch of 16 already-decoded images of each directory: Pillow resize to 512 + FaceParsing.normalise +
              its uploads (the host path's share that is not decoding) against one ImageIngest.parse_input call on pixels that are
              already on the device (wall clock with a synchronisation, and device events around the call)
The outputs of the two sides are compared once per directory: the label files' pixels are equal, the codes agree within 1e-5.
No ratio is fixed in advance: each row carries the gap between the medians beside the yardstick's own spread (max - min).

    python tools/ingest_time.py [--repeats 20] [--out profiles/ingest.json] [--small]

--small: 32 / 32 / 2 files and fewer repeats, to try the tool out.
"""
import argparse
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


def spread(v, unit):
    v = sorted(v)
    return {f'median_{unit}': round(float(np.median(v)), 3), f'min_{unit}': round(v[0], 3), f'max_{unit}': round(v[-1], 3)}


def compare(host, dev, unit, more_is_better):
    """The verdict by the spreads, and the gap of the medians beside the yardstick's own spread."""
    h, d = [host[f'{k}_{unit}'] for k in ('min', 'median', 'max')], [dev[f'{k}_{unit}'] for k in ('min', 'median', 'max')]
    if more_is_better:
        verdict = 'device faster' if d[0] > h[2] else 'host faster' if d[2] < h[0] else 'within the spread'
    else:
        verdict = 'device faster' if d[2] < h[0] else 'host faster' if d[0] > h[2] else 'within the spread'
    gap, own = d[1] - h[1], h[2] - h[0]
    return {'verdict': verdict, f'gap_{unit}': round(gap, 3), f'yardstick_spread_{unit}': round(own, 3), 'gap_exceeds_yardstick_spread': abs(gap) > own,
            'device_over_host': round(d[1] / h[1], 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ingest.json'))
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    from PIL import Image
    from jpeg_decode_time import photo
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd.hair_editor import HairEditor
    from ctrlhair_amd.ingest import ImageIngest
    sync = torch.cuda.synchronize
    batch = 16
    counts = (32, 32, 2) if args.small else (256, 256, 16)
    repeats = min(args.repeats, 3) if args.small else args.repeats
    he = HairEditor(True, True, weights='procedural', device=0, img_size=256, max_batch=batch)
    fp = he.face_parsing
    tmp = tempfile.mkdtemp(prefix='ingest_time_')
    specs = [('jpeg1024', counts[0], 1024, 1024, '.jpg', ('masks', 'codes')), ('png256', counts[1], 256, 256, '.png', ('masks', 'codes')),
             ('photo12mp', counts[2], 3000, 4000, '.jpg', ('masks',))]
    out = {'what': 'dataset masks / codes end to end, decode=host (the parent commit: the yardstick) against decode=device (device decode + '
                   'ch_ingest_images / ch_ingest_labels), images per second; and the ingest step alone, ms per batch of 16; median (min - max), '
                   'the two sides alternating in one loop; one session', 'repeats': repeats, 'batch': batch,
           'device': torch.cuda.get_device_name(0), 'jobs': [], 'ingest_alone': []}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)

    for name, count, H, W, ext, jobs in specs:
        img_dir = os.path.join(tmp, name, 'images')
        os.makedirs(img_dir)
        distinct = [photo(H, W, seed=31 * k + H) for k in range(min(count, batch))]      # 16 distinct images, written under `count` names
        for k in range(count):
            Image.fromarray(distinct[k % len(distinct)]).save(os.path.join(img_dir, f'{k:04d}{ext}'), **({'quality': 90} if ext == '.jpg' else {}))
        file_bytes = sum(os.path.getsize(os.path.join(img_dir, n)) for n in os.listdir(img_dir))
        label_dir = {m: os.path.join(tmp, name, 'label_' + m) for m in ('host', 'device')}
        code_dir = {m: os.path.join(tmp, name, 'codes_' + m) for m in ('host', 'device')}

        def run(job, mode):
            stats = {}
            sync()
            t0 = time.perf_counter()
            if job == 'masks':
                n = len(D.extract_masks(he, img_dir, label_dir[mode], batch, decode=mode, stats=stats))
            else:
                n = len(D.encode_sean_codes(he, img_dir, label_dir['host'], code_dir[mode], 'ds', batch, decode=mode, stats=stats))
            sync()
            dt = time.perf_counter() - t0
            assert n == count and stats['fallbacks'] == 0
            return n / dt

        for job in jobs:
            acc = {'host': [], 'device': []}
            for rep in range(-1, repeats):
                for mode in ('host', 'device'):
                    v = run(job, mode)
                    if rep >= 0:
                        acc[mode].append(v)
            if job == 'masks':
                equal = all(np.array_equal(D.read_gray(os.path.join(label_dir['host'], n)), D.read_gray(os.path.join(label_dir['device'], n)))
                            for n in os.listdir(label_dir['host']))
                agree = {'label_pixels_equal': bool(equal)}
            else:
                codes = {m: D.merge_pickle_dir_to_dict(code_dir[m], os.path.join(tmp, name, m + '.pkl')) for m in ('host', 'device')}
                agree = {'codes_max_abs_diff': float(max(np.abs(codes['host'][k] - codes['device'][k]).max() for k in codes['host']))}
            row = {'directory': name, 'job': job, 'files': count, 'H': H, 'W': W, 'format': ext[1:], 'file_bytes': file_bytes,
                   'host': spread(acc['host'], 'img_per_s'), 'device': spread(acc['device'], 'img_per_s')}
            row.update(compare(row['host'], row['device'], 'img_per_s', True))
            row.update(agree)
            out['jobs'].append(row)
            print(json.dumps(row), flush=True)
            flush()

        # the ingest step alone on one batch of this directory
        host_px = distinct[:batch] if len(distinct) >= batch else (distinct * batch)[:batch]
        dev_px = [torch.from_numpy(a).to(he.device) for a in host_px]
        ing = ImageIngest(fp.handle, fp.device)
        lut = fp.ingest_lut()
        want = torch.cat([fp.normalise(np.asarray(Image.fromarray(a).resize((512, 512), Image.BILINEAR))) for a in host_px], dim=0)
        assert torch.equal(ing.parse_input(dev_px, 512, lut=lut), want), name
        t = {'host': [], 'device': [], 'device_events': []}
        for rep in range(-2, repeats):
            sync()
            t0 = time.perf_counter()
            x = torch.cat([fp.normalise(np.asarray(Image.fromarray(a).resize((512, 512), Image.BILINEAR))) for a in host_px], dim=0)
            sync()
            t1 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = ing.parse_input(dev_px, 512, lut=lut)
            e1.record()
            sync()
            t2 = time.perf_counter()
            if rep >= 0:
                t['host'].append((t1 - t0) * 1e3)
                t['device'].append((t2 - t1) * 1e3)
                t['device_events'].append(e0.elapsed_time(e1))
            del x, y
        row = {'directory': name, 'batch': batch, 'H': H, 'W': W, 'to': 512, 'host_resize_normalise_upload': spread(t['host'], 'ms'),
               'device_parse_input': spread(t['device'], 'ms'), 'device_parse_input_events': spread(t['device_events'], 'ms')}
        row.update(compare(row['host_resize_normalise_upload'], row['device_parse_input'], 'ms', False))
        out['ingest_alone'].append(row)
        print(json.dumps(row), flush=True)
        flush()
        del dev_px, want
        shutil.rmtree(os.path.join(tmp, name))
    shutil.rmtree(tmp, ignore_errors=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
