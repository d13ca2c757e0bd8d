#!/usr/bin/env python3
"""Golden vectors for the BATCHED Poisson blending step: outputs of the REFERENCE function (imported in place, exactly as
make_poisson_golden.py imports it; numpy + scipy only) on four seeded 64x64 cases of one shape, stacked.  Run in the build
container:

    python tests/golden/make_poisson_batch_golden.py        -> tests/golden/poisson_batch_golden.npz

The masks differ so that a batched CG solve converges raggedly: a blob away from the border, an all-zero mask (nothing to
solve in the interior: converges in the first iterations), a mask that touches the image border, and a hair-like mask
(solve everywhere but a blob).  Arrays: src, tgt, out uint8 [4,64,64,3]; mask uint8 [4,64,64]; names."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_poisson_golden import blob_mask, poisson_blending, smooth_image       # noqa: E402  (reference, read-only)

S = 64


def main():
    rng = np.random.default_rng(20261016)
    masks = {'blob_inside': blob_mask(rng, S, S, 30, 28, 14, 17),
             'all_zero': np.zeros((S, S), np.uint8),
             'touches_border': blob_mask(rng, S, S, 0, 30, 26, 22, invert=True),
             'hair_like': blob_mask(rng, S, S, 20, 32, 18, 22, invert=True)}
    src = np.stack([smooth_image(rng, S, S) for _ in masks])
    tgt = np.stack([smooth_image(rng, S, S) for _ in masks])
    mask = np.stack(list(masks.values()))
    out = np.stack([poisson_blending(src[i].copy(), tgt[i].copy(), mask[i].copy()[..., None], with_gamma=True)
                    for i in range(len(masks))])
    np.savez_compressed(os.path.join(HERE, 'poisson_batch_golden.npz'), src=src, tgt=tgt, mask=mask, out=out.astype(np.uint8),
                        names=np.array(list(masks)))
    print('wrote', len(masks), 'cases')


if __name__ == '__main__':
    main()
