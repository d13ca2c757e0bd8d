"""The miss path of the label memo (option sean.label_memo): the headline generator job of bench.py -- exact f32, B = 16, 512 x 512, ngf = 64,
blocky labels -- with TWO label sets alternating call by call, so that no call finds the maps of the call before it.

    python tools/label_memo_bench.py [--labels alternate|pairs|same] [--codes same|alternate] [--steps K] [--warmup W] [--opt key=value ...]

Timed as bench.py times a leg: warm-up, synchronise, one event per step on the launch stream, synchronise; step_ms = the intervals between
the events.  Prints one JSON line {labels, codes, step_ms: {median, p10, p90, n}, images_per_s, memo: [calls, hits] | null, spade_memo:
[stores, loads] | null, code_memo: [calls, hits] | null}.  --labels same keeps one label set (the headline itself; with --opt sean.label_memo=0 it measures the library without the
memo).  --labels pairs brings every label set twice -- L, L, L', L', ... -- so that every second call is a label hit that stores the SPADE
memo's accumulators (option sean.spade_memo) and none ever loads them: its worst case; the line then also holds the medians of the first and
of the second calls of the pairs (step_ms_first, step_ms_second).  --codes alternate brings TWO sets of style codes call by call, the miss
path of the code memo (option sean.code_memo); with --labels it times the four hit / miss combinations of the two memos.  A library older than a memo runs too: its counters then read null.
Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctrlhair_amd import procedural as P                 # noqa: E402
from ctrlhair_amd.sean.generator import SeanGenerator    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--labels', choices=('alternate', 'pairs', 'same'), default='alternate')
    ap.add_argument('--codes', choices=('same', 'alternate'), default='same')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--opt', action='append', default=[], help='key=value pairs for ch_set_option, before ch_finalize')
    a = ap.parse_args()
    B, S = a.batch, a.size
    opts = {k: int(v) for k, v in (kv.split('=') for kv in a.opt)}
    gen = SeanGenerator(0, f16x3=0, options=opts).load_state_dict(P.sean_state_dict(0, a.ngf), max_batch=B, max_size=S)
    dev = gen.device
    csets = [torch.from_numpy(P.style_codes(B, first=first)).to(dev) for first in ((0,) if a.codes == 'same' else (0, B))]
    noise = torch.from_numpy(P.noise_planes(B, S, a.ngf)).to(dev)
    sets = [torch.from_numpy(P.blocky_labels(B, S, first=first)).to(dev) for first in ((0,) if a.labels == 'same' else (0, B))]
    rep = 2 if a.labels == 'pairs' else 1          # calls in a row with one label set
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    for i in range(a.warmup):
        gen.generate(sets[i // rep % len(sets)], csets[i % len(csets)], noise, out=out)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    for i in range(a.steps):
        marks[i].record()
        gen.generate(sets[(a.warmup + i) // rep % len(sets)], csets[(a.warmup + i) % len(csets)], noise, out=out)
    marks[a.steps].record()
    torch.cuda.synchronize()
    ms = np.asarray([marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)], dtype=np.float64)
    assert bool(torch.isfinite(out).all())
    stats, spade = getattr(gen.handle, 'sean_label_memo_stats', None), getattr(gen.handle, 'sean_spade_memo_stats', None)
    code = getattr(gen.handle, 'sean_code_memo_stats', None)

    def summary(v):
        return {'median': round(float(np.median(v)), 3), 'p10': round(float(np.percentile(v, 10)), 3), 'p90': round(float(np.percentile(v, 90)), 3), 'n': int(v.size)}
    line = {'labels': a.labels, 'codes': a.codes, 'options': opts, 'step_ms': summary(ms)}
    if a.labels == 'pairs':
        first = (a.warmup + np.arange(a.steps)) % 2 == 0
        line['step_ms_first'], line['step_ms_second'] = summary(ms[first]), summary(ms[~first])
    line.update({'images_per_s': round(B * a.steps / (ms.sum() / 1e3), 2), 'memo': list(stats()) if stats else None,
                 'spade_memo': list(spade()) if spade else None, 'code_memo': list(code()) if code else None})
    print(json.dumps(line), flush=True)
    gen.handle.close()


if __name__ == '__main__':
    main()
