#!/usr/bin/env python3
"""Census of the boundary quads of the Winograd ACE levels on the host: the classification rules of csrc/ace_sparse.hip (interior,
straight-edge and frame pixels) restated in numpy.  Per level and label set: boundary quads per sample with sean.edge alone, how many of
them lie on the two-pixel frame, and what sean.frame leaves.  The rules are a restatement: when ace_classify_kernel changes, this file has to be
changed with it by hand (tests/test_hip_frame_rows.py checks the kernel, not this tool).  Usage: frame_census.py [--size 512] [--samples 4] [--batch 16]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def classify(lab, frame):
    """u5-style map of one label map [H][W]: True where the pixel stays a boundary pixel."""
    H, W = lab.shape
    L = np.full((H + 4, W + 4), -1, np.int32)               # -1: outside the image (a 255 inside stays 255)
    L[2:-2, 2:-2] = lab
    win = np.stack([L[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)]).reshape(5, 5, H, W)      # [dy][dx]
    c = lab.astype(np.int32)
    interior = (c < 19) & (win == c).all(axis=(0, 1))
    inside = win >= 0
    full = inside.all(axis=(0, 1))
    edge = np.zeros((H, W), bool)
    for v in (win, win.transpose(1, 0, 2, 3)):              # v[i][j]: line j along the split direction
        lines_uniform = (v == v[0:1]).all(axis=(0, 1))
        l = v[0]
        A, Bl = l[0], l[4]
        ok = full & lines_uniform & (A < 19) & (Bl < 19) & (A != Bl) & (A >= 0) & (Bl >= 0)
        mono = np.ones((H, W), bool)                        # A..A B..B: once B is seen, no A follows
        for j in range(1, 4):
            mono &= ((l[j] == A) | (l[j] == Bl)) & ~((l[j] == A) & (l[j - 1] == Bl))
        edge |= ok & mono
    edge &= ~interior
    fr = np.zeros((H, W), bool)
    if frame:
        cut_x = ~inside[2].all(axis=0)                      # some column of the window is outside (the centre row tells)
        cut_y = ~inside[:, 2].all(axis=0)                   # some row
        same = (~inside | (win == c)).all(axis=(0, 1))
        fr = (cut_x != cut_y) & same & (c < 19) & ~interior & ~edge
    return ~(interior | edge | fr)


def quads(bnd):
    H, W = bnd.shape
    q = bnd.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))
    on_frame = np.zeros_like(q)
    on_frame[0, :] = on_frame[-1, :] = on_frame[:, 0] = on_frame[:, -1] = True
    return int(q.sum()), int((q & on_frame).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--samples', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    a = ap.parse_args()
    from ctrlhair_amd import procedural as P
    S = a.size
    sets = {'blocky': P.blocky_labels(a.batch, S)[:a.samples], 'face': np.stack([P.face_like_labels(S, 40 + b) for b in range(a.samples)])}
    print('| labels | level | boundary quads, sean.frame = 0 | of them on the frame | boundary quads, sean.frame = 1 | ratio |')
    print('|---|---|---|---|---|---|')
    for name, labs in sets.items():
        for div in (4, 2, 1):
            r = S // div
            n0 = f0 = n1 = 0
            for lab in labs:
                lv = lab[::div, ::div]                      # nearest down-sampling of the label map (generator.py:53 in reverse)
                q0, fq = quads(classify(lv, False))
                q1, _ = quads(classify(lv, True))
                n0 += q0; f0 += fq; n1 += q1
            k = len(labs)
            print(f'| {name} | {r} | {n0 / k:.0f} | {f0 / k:.0f} | {n1 / k:.0f} | {n1 / max(n0, 1):.2f} |')


if __name__ == '__main__':
    main()
