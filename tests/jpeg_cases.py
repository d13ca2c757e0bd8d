"""The JPEG encoder's test images, shared by tests/test_jpeg.py (oracle against Pillow's recorded files) and tests/test_hip_jpeg.py
(device against oracle).  A case is (H, W, content, quality, mode); mode '420' / '444' are RGB at that subsampling, 'grey' is one channel.

Sizes: one pixel; smaller than a block in both axes; exactly a block; exactly a 4:2:0 MCU; odd in both axes with a dummy luma column and
row at 4:2:0 (17x23: 3 block rows in 2 MCU rows); 33x130 (an odd block count in both axes, 17 block columns: the last MCU column is half
dummy); several MCU rows (64x80); 264x520 (thousands of blocks; its noise scan is over 64 KiB: more than 256 of the stuffing pass's
256-byte segments); 424x424 at 4:4:4 (8427 blocks: more than the 8192 = 256 groups x 32 blocks that one round of the bit-offset scan covers).
"""
import numpy as np

CONTENTS = ('noise', 'smooth', 'flat', 'checker', 'cos77')
QUALITIES = (1, 25, 75, 90, 100)
MODES = ('420', '444', 'grey')
SMALL_SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 130), (64, 80))
SUBSAMPLING = {'420': 2, '444': 0, 'grey': 2}      # Pillow's numbering; ignored for grey


def image(H, W, content, mode, seed=0):
    """uint8 [H,W,3], or [H,W] for mode 'grey'."""
    C = 1 if mode == 'grey' else 3
    rng = np.random.default_rng([seed, H, W, C, CONTENTS.index(content)])
    y, x = np.mgrid[0:H, 0:W]
    if content == 'noise':
        img = rng.integers(0, 256, (H, W, C))
    elif content == 'smooth':
        img = np.stack([127.5 + 127.5 * np.sin(x / (9.0 + 4 * c) + c) * np.cos(y / (13.0 - 3 * c)) for c in range(C)], axis=-1)
    elif content == 'flat':
        img = np.broadcast_to(np.array([200, 30, 90])[:C], (H, W, C))
    elif content == 'checker':                           # 4x4 cells of 0 or 255: the largest DC steps and AC terms
        cells = rng.integers(0, 2, ((H + 3) // 4, (W + 3) // 4, C)) * 255
        img = np.repeat(np.repeat(cells, 4, axis=0), 4, axis=1)[:H, :W]
    elif content == 'cos77':                             # every block only its highest-frequency coefficient: no EOB, three ZRLs
        v = 128 + 127 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
        img = np.repeat(v[..., None], C, axis=-1)
    else:
        raise ValueError(content)
    img = np.clip(np.rint(np.asarray(img, np.float64)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0] if C == 1 else img)


def _cases():
    out = []
    for i, (H, W) in enumerate(SMALL_SIZES):
        for m, mode in enumerate(MODES):
            for k, q in enumerate(QUALITIES):
                out.append((H, W, CONTENTS[(i + m + k) % len(CONTENTS)], q, mode))
    out += [(264, 520, 'noise', 75, '420'), (264, 520, 'checker', 25, '444'), (264, 520, 'smooth', 90, 'grey'), (264, 520, 'cos77', 25, '420'),
            (424, 424, 'checker', 1, '444'), (424, 424, 'smooth', 75, '420')]
    return out


CASES = _cases()


def case_id(case):
    H, W, content, q, mode = case
    return f'{H}x{W}-{content}-q{q}-{mode}'


def case_image(case):
    H, W, content, _, mode = case
    return image(H, W, content, mode)
