"""Inputs of the matte paste-back tests (test code only): photos, edits and plans of tests/unalign_cases.py with weight maps of their
own -- a disc of 255, a stretch of random values and a zero band -- and the (radius, eps) grid.  tests/test_matte.py checks the
oracle on them (CPU), tests/test_hip_matte.py the library (GPU); the float64 oracle result of a case is computed once and shared."""
import functools

import numpy as np

from tests import matte_oracle as MO
from tests import unalign_cases as UC

# plan of unalign_cases -> why it is here
PLANS = {
    'e_batch_feather': 'N = 3, s = 0.43: a domain of about 75 px',
    'b_minify': 's = 3.2: several crop pixels per photo pixel',
    'c_padded': 'bbox clipped by the photo',
    'f_origin': 'bbox at row and column 0, partial tiles',
}

# name -> (plan, radius, eps)
CASES = {f'{plan}-r{r}-eps{eps:g}': (plan, r, eps) for plan in PLANS for r in (1, 3, 8) for eps in (1e-2, 1e-4)}
CASES['e_batch_feather-r64-eps0.0001'] = ('e_batch_feather', 64, 1e-4)      # the window exceeds the domain: every window is clipped
CASES['e_batch_feather-r1-eps1e-06'] = ('e_batch_feather', 1, 1e-6)         # the worst case for float32 moments
WORST = 'e_batch_feather-r1-eps1e-06'


@functools.lru_cache(maxsize=None)
def weight_map(plan):
    """uint8 [S,S]: a disc of 255 around the centre, a stretch of random values across it, and a zero band on top."""
    S = int(UC.inputs(plan)['plan_u']['output_size'])
    rng = np.random.RandomState(S + len(plan))
    j, i = np.mgrid[0:S, 0:S]
    w = np.where((i - 0.55 * S) ** 2 + (j - 0.5 * S) ** 2 < (0.36 * S) ** 2, 255, 0).astype(np.uint8)
    w[S // 2: S // 2 + max(S // 8, 2), S // 4: 3 * S // 4] = rng.randint(0, 256, size=(max(S // 8, 2), 3 * S // 4 - S // 4))
    w[: S // 5] = 0                                   # a band where the photo must come through untouched
    return w


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict: unalign_cases.inputs(plan) with weight replaced, plus radius and eps."""
    plan, r, eps = CASES[name]
    return dict(UC.inputs(plan), weight=weight_map(plan), radius=r, eps=eps)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(out uint8 [N,H,W,3], alpha float32 [bh,bw]) of the float64 oracle."""
    c = inputs(name)
    return MO.paste_back_matte(c['photo'], c['edits'], c['plan_u'], c['weight'], c['feather'], c['radius'], c['eps'])


def compare(name, got, got_alpha):
    """Figures of the library's (out uint8 [N,H,W,3], alpha float32 [bh,bw]) against the oracle."""
    c = inputs(name)
    ref, alpha = oracle(name)
    x0, y0, x1, y1 = c['plan_u']['bbox']
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    untouched = np.ones(c['photo'].shape[:2], bool)
    untouched[y0:y1, x0:x1] = alpha == 0
    return {'alpha_max': float(np.abs(got_alpha.astype(np.float64) - alpha.astype(np.float64)).max()),
            'zero_set_equal': bool(((got_alpha == 0) == (alpha == 0)).all()),
            'max': int(d.max()), 'share': float((d[:, y0:y1, x0:x1].max(axis=-1) > 0).mean()),
            'photo_kept': bool((got[:, untouched] == c['photo'][untouched]).all())}
