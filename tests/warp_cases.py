"""Shared set-up of the mask-warp tests: the synthetic cases of tests/golden/warp_cases.npz with their host meshes."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS_PX = 672 * 672
NEAR_EDGE = 1e-6             # a barycentric this close to 0 may fall on either side of a triangle edge
NEAR_EDGE_CAP = 0.001        # ... on at most 0.1 % of the canvas
HARD_DU_PX = 0.05            # ARAP: the output is sampled at 1/32 px


@functools.lru_cache(maxsize=None)
def cases():
    """-> list of dicts(hair, face, hair_lm, face_lm, V, F, b, bc) for the four fixture pairs (scipy meshes)."""
    from ctrlhair_amd import warping as W
    z = np.load(os.path.join(GOLDEN, 'warp_cases.npz'))
    out = []
    for i in range(len(z['hair_lm'])):
        nodes, targets = W.build_nodes(z['hair_lm'][i], z['face_lm'][i])
        V, F, b = W.build_mesh(nodes)
        out.append(dict(hair=z['hair_labels'][i], face=z['face_labels'][i], hair_lm=z['hair_lm'][i], face_lm=z['face_lm'][i],
                        V=V, F=F, b=b, bc=targets.astype(np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def oracle(i):
    """Oracle end to end on case i -> (labels, uv, U float32)."""
    from tests import warp_oracle as O
    c = cases()[i]
    return O.warp(c['hair'], c['face'], c['V'], c['F'], c['b'], c['bc'])


def boundary_band(hair_mask):
    """The one-pixel band around the boundary of a 0/1 mask: pixels with a 4-neighbour of the other value."""
    m = np.asarray(hair_mask).astype(bool)
    d = np.zeros_like(m)
    d[1:] |= m[1:] != m[:-1]
    d[:-1] |= m[1:] != m[:-1]
    d[:, 1:] |= m[:, 1:] != m[:, :-1]
    d[:, :-1] |= m[:, 1:] != m[:, :-1]
    return d


@functools.lru_cache(maxsize=None)
def triangle_meshes():
    """The two meshes Shewchuk's Triangle (-q30) made for pairs 0 and 1 (tests/golden/warp_triangle_meshes.npz), as case dicts."""
    m = np.load(os.path.join(GOLDEN, 'warp_triangle_meshes.npz'))
    return [dict(cases()[i], V=m[f'V{i}'], F=m[f'F{i}'], b=np.arange(273, dtype=np.int32), bc=m[f'bc{i}']) for i in (0, 1)]
