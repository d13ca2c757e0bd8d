"""Inputs of the paste-back tests (test code only): the smallest photos and plans that reach every branch of ch_face_unalign, built
from the fixture generators of tests/align_oracle.py.  tests/test_unalign.py runs the float32 emulation of the oracle on them (CPU),
tests/test_hip_unalign.py the library (GPU); the float64 oracle result of a case is computed once and shared."""
import functools

import numpy as np

from ctrlhair_amd import alignment as AL
from tests import align_oracle as AO
from tests import unalign_oracle as UO

# name -> (seed, photo height, width, eye centre (x, y), eye distance, angle, S, transform_size, N, weight map?, feather_px (None = S / 16))
# The quad's side is about 4.14 eye distances.
CASES = {
    'a_magnify': (31, 160, 200, (100.0, 72.0), 18.0, 17.0, 32, 128, 1, False, None),        # s = 0.43: 6 x 6 interpolation
    'b_minify': (32, 160, 200, (96.0, 70.0), 9.7, -23.0, 128, 256, 1, False, None),         # s = 3.2: 20-tap loops
    'c_padded': (33, 160, 200, (34.0, 30.0), 18.0, 11.0, 32, 128, 1, False, None),          # quad partly outside: pad, clipped bbox
    'd_shrink': (34, 200, 240, (120.0, 90.0), 20.0, -8.0, 16, 64, 1, False, None),          # 83-px quad at S = 16: shrink 2
    'e_batch_hard': (35, 160, 200, (100.0, 72.0), 18.0, 17.0, 32, 128, 3, True, 0.0),       # N = 3, weight map, hard edge
    'e_batch_feather': (35, 160, 200, (100.0, 72.0), 18.0, 17.0, 32, 128, 3, True, None),   # the same with the default feather
    'f_origin': (36, 150, 170, (38.0, 30.0), 19.0, 0.0, 48, 96, 2, False, None),            # bbox starts at row 0 / column 0, partial tiles
    'h_lds': (37, 64, 64, (32.0, 30.0), 2.55, 31.0, 128, 128, 1, False, None),              # s = 12: 73 taps, more than 64 KiB of LDS
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict: photo [H,W,3], edits [N,S,S,3], weight [S,S] or None, feather (float), plan (align_plan), plan_u (unalign_plan)."""
    seed, H, W, centre, eye, angle, S, T, N, has_w, feather = CASES[name]
    photo = AO.make_photo(seed, H, W)
    lm = AO.make_landmarks(seed + 100, centre, eye, angle)
    plan = AL.align_plan(lm, H, W, S, T)
    rng = np.random.RandomState(seed + 200)
    edits = np.stack([AO.make_photo(seed + 300 + n, S, S) for n in range(N)])
    weight = rng.randint(0, 256, size=(S, S)).astype(np.uint8) if has_w else None
    if weight is not None:
        weight[: S // 4] = 0                          # a stretch where the photo must come through untouched
        weight[S // 4: S // 2, : S // 2] = 255
    return {'photo': photo, 'lm': lm, 'edits': edits, 'weight': weight, 'feather': S / 16.0 if feather is None else feather, 'plan': plan,
            'plan_u': AL.unalign_plan(plan, H, W)}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(out uint8 [N,H,W,3], alpha float64 [H,W]) of the float64 oracle."""
    c = inputs(name)
    return UO.paste_back(c['photo'], c['edits'], c['plan_u'], c['weight'], c['feather'], return_alpha=True)


def compare(name, got):
    """Figures of `got` (uint8 [N,H,W,3]) against the oracle: max grey-level difference, share of differing pixels inside bbox, and
    whether everything outside bbox or with alpha == 0 equals the photo."""
    c = inputs(name)
    ref, alpha = oracle(name)
    x0, y0, x1, y1 = c['plan_u']['bbox']
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    inside = d[:, y0:y1, x0:x1].max(axis=-1)
    untouched = alpha == 0
    return {'max': int(d.max()), 'share': float((inside > 0).mean()), 'photo_kept': bool((got[:, untouched] == c['photo'][untouched]).all())}
