"""Host oracle of the face alignment (test code only): runs a plan of ctrlhair_amd.alignment.align_plan with Pillow, numpy and scipy
THEMSELVES -- Image.resize(LANCZOS), Image.crop, np.pad, scipy.ndimage.gaussian_filter, np.median, Image.transform(QUAD, BILINEAR)
-- stage by stage, so that each device stage has something exact to be compared with.  Also generates the fixture photos and
landmarks (pure numpy, from a seed; tests/golden/make_align_golden.py records their SHA-256)."""
import hashlib

import numpy as np
from PIL import Image

LANCZOS = Image.LANCZOS


def resize(img, size):
    """Image.resize((w, h), LANCZOS) of a uint8 [H,W,C] / [H,W] array."""
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((int(size[0]), int(size[1])), LANCZOS))


def feather_ramps(h, w, pad):
    """The feather mask of the padding branch, float64 [h,w,1]: 0 inside the photo, rising to 1 at the padded border.  The ramps are
    float32 pixel indices divided by int64 pad widths, which numpy 2 promotes to float64."""
    left, top, right, bottom = np.asarray(pad, np.int64)
    rows, cols = np.arange(h).reshape(h, 1, 1), np.arange(w).reshape(1, w, 1)
    ramp_x = np.minimum(np.float32(cols) / left, np.float32(w - 1 - cols) / right)
    ramp_y = np.minimum(np.float32(rows) / top, np.float32(h - 1 - rows) / bottom)
    return np.maximum(1.0 - ramp_x, 1.0 - ramp_y)


def pad_feather(img, pad, qsize):
    """The padding branch on a uint8 [H,W,3] array: pad = (left, top, right, bottom), blur sigma = 0.02 qsize -> uint8 padded image:
    reflect pad in float32, blend towards the Gaussian blur where the mask exceeds -1/3, then towards the per-channel median by the
    mask, both in place (float64 arithmetic stored back to float32), round, clip."""
    from scipy.ndimage import gaussian_filter
    left, top, right, bottom = (int(v) for v in pad)
    canvas = np.pad(np.asarray(img).astype(np.float32), ((top, bottom), (left, right), (0, 0)), mode='reflect')
    mask = feather_ramps(canvas.shape[0], canvas.shape[1], pad)
    sigma = qsize * 0.02
    blurred = gaussian_filter(canvas, [sigma, sigma, 0])
    canvas += (blurred - canvas) * np.clip(mask * 3.0 + 1.0, 0.0, 1.0)
    canvas += (np.median(canvas, axis=(0, 1)) - canvas) * np.clip(mask, 0.0, 1.0)
    return np.clip(np.rint(canvas), 0, 255).astype(np.uint8)


def quad_warp(img, corners, transform_size, output_size):
    """Image.transform((T, T), QUAD, corners, BILINEAR) then resize((S, S), LANCZOS) when S < T, of a uint8 [H,W,3] array."""
    im = Image.fromarray(np.ascontiguousarray(img)).transform((transform_size, transform_size), Image.QUAD,
                                                              np.asarray(corners, np.float64).flatten(), Image.BILINEAR)
    if output_size < transform_size:
        im = im.resize((output_size, output_size), LANCZOS)
    return np.asarray(im)


def run_plan(img, plan, stages=None):
    """The whole plan on the host.  stages (optional dict) receives 'shrunk', 'cropped', 'padded' (the uint8 image after that step,
    where the step ran) and 'source' (what the transform reads)."""
    stages = {} if stages is None else stages
    img = np.ascontiguousarray(img)
    if plan['shrink'] > 1:
        img = stages['shrunk'] = resize(img, plan['resized'])
    x0, y0, x1, y1 = plan['crop']
    if plan['cropped']:
        img = stages['cropped'] = np.ascontiguousarray(img[y0:y1, x0:x1])
    if plan['padded']:
        img = stages['padded'] = pad_feather(img, plan['pad'], plan['qsize'])
    stages['source'] = img
    return quad_warp(img, plan['quad'] + 0.5, plan['transform_size'], plan['output_size'])


# ---- fixture inputs -------------------------------------------------------------------------------------------------------------
def make_photo(seed, height, width):
    """A deterministic RGB photo uint8 [height,width,3]: smooth colour waves, a blocky patchwork and a band of per-pixel noise, so
    that interpolation, rounding and the blur all have something to disagree about."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:height, :width].astype(np.float64)
    img = np.zeros((height, width, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.004, 0.03, 2).tolist() + [rng.uniform(0, 6.28)]
        img[..., c] = 127.5 + 90.0 * np.sin(xx * fx + yy * fy + ph) * np.cos(yy * fx * 0.7 - xx * fy * 0.4)
    bs = 24
    blocks = rng.randint(-40, 41, size=((height + bs - 1) // bs, (width + bs - 1) // bs, 3))
    img += np.kron(blocks, np.ones((bs, bs, 1)))[:height, :width]
    band = slice(height // 3, height // 3 + max(height // 10, 8))
    img[band] += rng.randint(-60, 61, size=img[band].shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_landmarks(seed, centre, eye_dist, angle_deg):
    """68 plausible landmark pixels (float64): a frontal template (eyes at rows 36-47, mouth at 48-67) rotated by angle_deg about
    `centre` (x, y; the midpoint between the eyes) and scaled to `eye_dist` pixels between the eye centres, with a little jitter."""
    rng = np.random.RandomState(seed)
    t = np.zeros((68, 2))
    t[0:17] = np.stack([np.linspace(-1.1, 1.1, 17), 0.3 + 1.5 * np.sin(np.linspace(0, np.pi, 17))], 1)      # chin
    t[17:22] = np.stack([np.linspace(-0.85, -0.2, 5), np.full(5, -0.3)], 1)
    t[22:27] = np.stack([np.linspace(0.2, 0.85, 5), np.full(5, -0.3)], 1)
    t[27:31] = np.stack([np.zeros(4), np.linspace(0.0, 0.6, 4)], 1)
    t[31:36] = np.stack([np.linspace(-0.25, 0.25, 5), np.full(5, 0.75)], 1)
    ring = np.stack([np.cos(np.linspace(np.pi, -np.pi, 6, endpoint=False)), -0.5 * np.sin(np.linspace(np.pi, -np.pi, 6, endpoint=False))], 1)
    t[36:42] = [-0.5, 0.0] + 0.17 * ring
    t[42:48] = [0.5, 0.0] + 0.17 * ring
    a12 = np.linspace(np.pi, -np.pi, 12, endpoint=False)
    t[48:60] = [0.0, 1.15] + np.stack([0.42 * np.cos(a12), -0.16 * np.sin(a12)], 1)
    a8 = np.linspace(np.pi, -np.pi, 8, endpoint=False)
    t[60:68] = [0.0, 1.15] + np.stack([0.3 * np.cos(a8), -0.07 * np.sin(a8)], 1)
    t += rng.uniform(-0.01, 0.01, t.shape)
    a = np.deg2rad(angle_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (t @ R.T) * eye_dist + np.asarray(centre, np.float64)


# name -> (seed, height, width, eye centre (x, y), eye distance, angle, output_size, transform_size); chosen so that between them the
# reference takes every branch (make_align_golden.py asserts which)
CASES = {
    'plain_256': (11, 900, 800, (410.0, 400.0), 95.0, 7.0, 256, 4096),             # crop to a sub-window, no shrink, no pad
    'pad_topleft_512': (12, 700, 600, (150.0, 120.0), 90.0, -12.0, 512, 2048),      # face near the top and the left side: pad
    'shrink_256': (13, 2400, 1800, (900.0, 1050.0), 375.0, 4.0, 256, 4096),         # ~1500-px quad: shrink 2
    'shrink_pad_256': (14, 1700, 1500, (1100.0, 500.0), 300.0, 15.0, 128, 1024),    # shrink and pad (right / top) together
    'nocrop_1024': (15, 520, 520, (260.0, 238.0), 110.0, 0.0, 1024, 4096),          # the box covers the photo: no crop, no pad
    'pad_right_1024': (16, 640, 560, (430.0, 300.0), 100.0, 20.0, 1024, 4096),      # pad on one side at 1024
}


def case_inputs(name):
    seed, height, width, centre, eye_dist, angle, out_size, t_size = CASES[name]
    return make_photo(seed, height, width), make_landmarks(seed + 100, centre, eye_dist, angle), out_size, t_size


def sha256(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()
