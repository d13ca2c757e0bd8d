"""Times a direction search per candidate -> profiles/direction_search.json.  For --candidates candidates x --images images x --values
slider values at 256 x 256 (procedural ngf = 64 weights), texture and shape, in one session, median (min - max) of --repeats runs:
  (a) yardstick: the reference-shaped loop on the batch-1 API -- Backend.set_input_img, then per value
      continue_change_with_direction + output() (blending off), the sheet pasted together in numpy (util/canvas_grid.py)
  (b) the job's path per candidate (ctrlhair_amd/directions.py), split into render (DirectionSearch.sweep), compose (sheet on the
      device), stats (ch_sweep_stats and its 16 integers per render to the host), download (the sheet) and PNG encoding (host zlib,
      reported apart); the one-off analysis of the images is given on its own
  (c) achieved bytes/s of ch_sheet_compose and ch_sweep_stats (device events) at the 60-render shape and at 512 x 512, with their share
      of the measured HBM copy rate.  Bytes are the ones the calls need by their shapes: compose reads every source once and writes
      every cell once; the statistics read both label maps and the image once (they touch the image only under hair, so this is an
      upper bound of their traffic).

    python tools/direction_time.py [--repeats 20] [--out profiles/direction_search.json]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X (8.0 TB/s specified)


def spread(ms):
    ms = sorted(ms)
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--candidates', type=int, default=4)
    ap.add_argument('--images', type=int, default=10)
    ap.add_argument('--values', type=int, default=6)
    ap.add_argument('--max-batch', type=int, default=20)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'direction_search.json'))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from ctrlhair_amd import directions as DS
    from ctrlhair_amd import hostutil as U
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import procedural_weights
    from ctrlhair_amd.pipeline import EditPipeline
    from ctrlhair_amd.ui.backend import Backend
    S, I, V, K = 256, args.images, args.values, args.candidates
    values = np.linspace(-2.5, 2.5, V)
    weights = procedural_weights(0, args.ngf)
    imgs_f = P.synthetic_images(I, S, seed=3)
    imgs_u8 = ((imgs_f.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).astype(np.uint8)
    sync = torch.cuda.synchronize
    rows = {}

    # ---- (a) the reference-shaped loop on the batch-1 API
    be = Backend(2.5, blending=False, weights=weights, device=0)

    def yardstick(att, d):
        step = 2 if att == 'shape' else 1
        canvas = np.full((step * I * S, (V + 1) * S, 3), 255, np.uint8)
        dd = d.to(be.device)
        for i in range(I):
            _, parsing = be.set_input_img(imgs_u8[i])
            canvas[step * i * S:(step * i + 1) * S, :S] = imgs_u8[i]
            if att == 'shape':
                canvas[(2 * i + 1) * S:(2 * i + 2) * S, :S] = parsing
            for v in range(V):
                be.continue_change_with_direction(att, dd, float(values[v]))
                canvas[step * i * S:(step * i + 1) * S, (v + 1) * S:(v + 2) * S] = be.output()
                if att == 'shape':
                    canvas[(2 * i + 1) * S:(2 * i + 2) * S, (v + 1) * S:(v + 2) * S] = U.mask_to_rgb(be.cur_mask)
        return canvas

    for att in ('texture', 'shape'):
        cands = [DS.candidate_direction(DS.DIMS[att], [], 0, k) for k in range(K)]
        yardstick(att, cands[0])                                             # warm-up
        per = []
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            for d in cands:
                yardstick(att, d)
            sync()
            per.append((time.perf_counter() - t0) * 1e3 / K)
        rows[att] = {'yardstick_per_candidate': spread(per)}
        print(att, 'yardstick', rows[att], flush=True)
    be.models.generator.handle.close()
    del be

    # ---- (b) the job's path
    pipe = EditPipeline(weights, device=0, img_size=S, max_batch=args.max_batch)
    dev_imgs = torch.from_numpy(imgs_f).cuda()
    DS.DirectionSearch(pipe, dev_imgs)                                       # warm-up
    sync()
    t0 = time.perf_counter()
    search = DS.DirectionSearch(pipe, dev_imgs)
    sync()
    analysis_ms = (time.perf_counter() - t0) * 1e3
    for att in ('texture', 'shape'):
        cands = [DS.candidate_direction(DS.DIMS[att], [], 0, k) for k in range(K)]
        stages = {k: [] for k in ('render', 'compose', 'stats', 'download', 'png_encode', 'total_without_png')}

        def candidate(d, acc):
            t = [time.perf_counter()]

            def mark():
                sync()
                t.append(time.perf_counter())
            images, masks = search.sweep(att, d, values)
            mark()
            sheet = search.sheet(att, images, masks)
            mark()
            st = search.stats(images, masks)
            DS.score(att, st, values, S, S)
            mark()
            arr = sheet.numpy()
            mark()
            Image.fromarray(arr).save(io.BytesIO(), format='PNG')
            mark()
            for k, a, b in (('render', 0, 1), ('compose', 1, 2), ('stats', 2, 3), ('download', 3, 4), ('png_encode', 4, 5),
                            ('total_without_png', 0, 4)):
                acc[k] = acc.get(k, 0.0) + (t[b] - t[a]) * 1e3

        candidate(cands[0], {})                                              # warm-up
        for _ in range(args.repeats):
            acc = {}
            for d in cands:
                candidate(d, acc)
            for k in stages:
                stages[k].append(acc[k] / K)
        rows[att]['job_per_candidate'] = {k: spread(v) for k, v in stages.items()}
        a, b = rows[att]['yardstick_per_candidate'], rows[att]['job_per_candidate']['total_without_png']
        rows[att]['gap_ms'] = round(a['median_ms'] - b['median_ms'], 4)
        rows[att]['larger_spread_ms'] = round(max(a['max_ms'] - a['min_ms'], b['max_ms'] - b['min_ms']), 4)
        rows[att]['job_below_yardstick_by_more_than_either_spread'] = bool(rows[att]['gap_ms'] > rows[att]['larger_spread_ms'])
        print(att, 'job', rows[att], flush=True)

    # ---- (c) the two kernels alone
    handle = search.handle
    kernels = []
    rng = np.random.default_rng(0)
    for size, hw in ((256, 256), (512, 256)):
        N = I * V
        src = torch.from_numpy(rng.uniform(-1, 1, (N, 3, size, size)).astype(np.float32)).cuda()
        lab = torch.from_numpy(rng.choice(np.array([13, 1, 2], np.uint8), size=(N, hw, hw))).cuda()
        sheet = DS.ContactSheet(handle, 'cuda:0', I, V + 1, size)
        cells = [(i, v + 1) for i in range(I) for v in range(V)]
        ref = torch.from_numpy(np.repeat(np.arange(I) * V, V).astype(np.int32)).cuda()
        cells_dev = torch.tensor(cells, dtype=torch.int32, device='cuda')
        out = torch.empty(N, 16, dtype=torch.int64, device='cuda')

        def compose():
            handle.call('ch_sheet_compose', src.data_ptr(), 0, N, size, size, cells_dev.data_ptr(), None, sheet.canvas.data_ptr(), I, V + 1,
                        size, size, 0, torch.cuda.current_stream().cuda_stream)

        def stats():
            handle.call('ch_sweep_stats', src.data_ptr(), 0, lab.data_ptr(), ref.data_ptr(), N, size, size, hw, hw, out.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)

        for name, fn, nbytes in (('ch_sheet_compose', compose, N * size * size * (12 + 3)),
                                 ('ch_sweep_stats', stats, N * (2 * size * size + size * size * 12))):
            fn()
            sync()
            ms = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            sp = spread(ms)
            rate = nbytes / (sp['median_ms'] * 1e-3)
            kernels.append({'call': name, 'renders': N, 'size': size, 'labels': hw, 'bytes': nbytes, **sp,
                            'bytes_per_s': round(rate, 1), 'share_of_hbm_copy_rate': round(rate / HBM_COPY_BYTES_PER_S, 4)})
            print(kernels[-1], flush=True)

    out = {'what': 'direction search per candidate: the batch-1 API loop of the reference (yardstick) against the batched job '
                   '(render, device sheet, device statistics, download), PNG encoding apart; one session',
           'repeats': args.repeats, 'candidates': K, 'images': I, 'values': V, 'size': S, 'ngf': args.ngf, 'max_batch': args.max_batch,
           'device': torch.cuda.get_device_name(0), 'analysis_once_ms': round(analysis_ms, 3), 'per_attribute': rows, 'kernels': kernels,
           'hbm_copy_bytes_per_s': HBM_COPY_BYTES_PER_S}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
