"""Inputs of the mask-warp tests -> tests/golden/warp_cases.npz (numpy only; run from the repository root:
`python tests/golden/make_warp_golden.py`).  Everything is synthetic and this project's own data:

* `template` float64 [81,2] in [0,1]: an 81-point face in the layout of the dlib 81-landmark model the reference uses (0-16 jaw,
  17-26 brows, 27-35 nose, 36-47 eyes, 48-67 mouth, 68-80 forehead line), drawn from arcs;
* `hair_lm`, `face_lm` float64 [4,81,2]: jittered / scaled / rotated / shifted variants of it, as (donor, face) pairs;
* `hair_labels`, `face_labels` uint8 [4,512,512]: CelebAMask-HQ label maps made of ellipses (skin 1, hair 13, background 0).  The
  hair of pair 0 touches the top edge of the image, that of pair 1 the top and the left edge, pair 3's donor has no hair.

Two more fixtures hold recorded DATA of the reference's tool chain and are not made by this script (the tools are not part of
this project; they were run once from a scratch copy, on pairs 0 and 1 above):

* warp_triangle_meshes.npz: V{0,1} float32 [n,2], F{0,1} int32 [m,3] (0-based), bc{0,1} float32 [273,2] -- the triangle.txt /
  correspondence.txt contents that step_3/generate_node.get_node + `triangle -q30` write for the nodes of build_nodes()
  (710 vertices / 1222 triangles and 695 / 1192);
* warp_meshcore_uv.npz: `U` float32 = the host oracle's ARAP result on mesh 0, and the UV image that mesh_core.cpp's
  render_colors_core (g++ -O2, no -ffast-math, no -march=native) drew from it with colours V / 671: rows 220..380 as float32
  values (`uv`, `uv_rows`), the coverage of the whole canvas as packed bits (`covered`), and the SHA-256 of the whole
  [672,672,2] float32 image (`sha256`).
"""
import os

import numpy as np


def template():
    p = np.zeros((81, 2))
    t = np.linspace(np.pi, 0, 17)                               # jaw: lower half of an ellipse, left to right
    p[0:17] = np.stack([0.5 + 0.27 * np.cos(t), 0.52 + 0.36 * np.sin(t)], 1)
    for k, cx in ((17, 0.385), (22, 0.615)):                    # brows
        x = np.linspace(-0.075, 0.075, 5)
        p[k:k + 5] = np.stack([cx + x, 0.40 - 0.02 * np.cos(x / 0.075 * np.pi / 2)], 1)
    p[27:31] = np.stack([np.full(4, 0.5), np.linspace(0.45, 0.58, 4)], 1)          # nose bridge
    p[31:36] = np.stack([np.linspace(0.445, 0.555, 5), 0.62 - 0.012 * np.cos(np.linspace(-1.5, 1.5, 5))], 1)
    for k, cx in ((36, 0.39), (42, 0.61)):                      # eyes: six points on an ellipse
        a = np.linspace(np.pi, -np.pi, 7)[:6]
        p[k:k + 6] = np.stack([cx + 0.05 * np.cos(a), 0.46 - 0.018 * np.sin(a)], 1)
    a = np.linspace(np.pi, -np.pi, 13)[:12]                     # mouth: outer 12, inner 8
    p[48:60] = np.stack([0.5 + 0.09 * np.cos(a), 0.73 - 0.035 * np.sin(a)], 1)
    a = np.linspace(np.pi, -np.pi, 9)[:8]
    p[60:68] = np.stack([0.5 + 0.055 * np.cos(a), 0.73 - 0.012 * np.sin(a)], 1)
    t = np.linspace(np.pi * 1.04, np.pi * 1.96, 13)             # forehead line: upper arc
    p[68:81] = np.stack([0.5 + 0.26 * np.cos(t), 0.42 + 0.27 * np.sin(t)], 1)
    return p


def variant(p, rng, scale, angle, shift, jitter):
    c, s = np.cos(angle), np.sin(angle)
    q = (p - 0.5) * scale @ np.array([[c, s], [-s, c]]) + 0.5 + np.asarray(shift)
    return q + rng.normal(0, jitter, q.shape)


def ellipse(cx, cy, rx, ry, n=512):
    y, x = np.mgrid[0:n, 0:n]
    return ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1


def labels(hair, face_c=(256, 280), n=512):
    m = np.zeros((n, n), np.uint8)
    for cx, cy, rx, ry in hair:
        m[ellipse(cx, cy, rx, ry)] = 13
    m[ellipse(face_c[0], face_c[1], 120, 160)] = 1
    return m


def main():
    rng = np.random.default_rng(20240817)
    t = template()
    hair_lm = np.stack([variant(t, rng, 1.00, 0.00, (0.00, 0.00), 0.004), variant(t, rng, 1.08, 0.06, (-0.02, 0.01), 0.004),
                        variant(t, rng, 0.92, -0.08, (0.03, 0.02), 0.004), variant(t, rng, 1.00, 0.03, (0.00, 0.00), 0.004)])
    face_lm = np.stack([variant(t, rng, 0.94, 0.05, (0.02, 0.03), 0.004), variant(t, rng, 0.97, -0.04, (0.02, -0.01), 0.004),
                        variant(t, rng, 1.05, 0.04, (-0.02, 0.00), 0.004), variant(t, rng, 1.03, -0.05, (0.01, 0.01), 0.004)])
    hair = np.stack([labels([(256, 150, 190, 170)]), labels([(200, 140, 230, 160), (90, 330, 60, 150)]),
                     labels([(256, 190, 170, 130), (400, 330, 50, 120)]), labels([])])
    face = np.stack([labels([(256, 200, 150, 120)], (262, 290)), labels([(256, 210, 140, 100)], (250, 285)),
                     labels([], (256, 280)), labels([(256, 200, 150, 120)], (256, 280))])
    assert (hair[0][0] == 13).any() and (hair[1][:, 0] == 13).any() and not (hair[3] == 13).any()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'warp_cases.npz')
    np.savez_compressed(out, template=t, hair_lm=hair_lm, face_lm=face_lm, hair_labels=hair, face_labels=face)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
