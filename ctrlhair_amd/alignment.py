"""FFHQ face alignment (external_code/crop.py:20-107 `recreate_aligned_images`; called by hair_editor.py:312-329 and
dataset_scripts/script_crop.py) on the HIP library.

`align_plan` is the host half: everything that depends only on the 68 landmarks and the photo's size, in float64, with the
operations in the order the reference evaluates them (the oriented quad decides every output pixel, so it must come out bit for
bit).  `FaceAligner.align` is the device half: ONE `ch_face_align` call per photo (csrc/face_align.hip) that shrinks, crops, pads
and feathers where the plan says so, evaluates Pillow's QUAD / BILINEAR transform fused into its Lanczos reduction, and returns
the aligned portrait as a device tensor.  It is exact against Pillow 8-bit, numpy and scipy ("Face alignment").  No CPU
fallback: without the library / a GPU `FaceAligner` raises.

Landmark detection is not part of this project: the 68 points come from the caller.
"""
import ctypes as C

import numpy as np

from .devop import DeviceOp

PLAN_LEN = 24                   # CH_ALIGN_PLAN_LEN
UNALIGN_PLAN_LEN = 16           # CH_UNALIGN_PLAN_LEN
UNALIGN_MAX_SCALE = 16          # CH_UNALIGN_MAX_SCALE
MAX_TRANSFORM = 16384           # CH_ALIGN_MAX_TRANSFORM
GAUSS_TRUNCATE = 4.0            # scipy.ndimage.gaussian_filter's default
MATTE_MAX_RADIUS = 64           # CH_MATTE_MAX_RADIUS
MATTE_DEFAULT_EPS = 1e-4
MATTE_CROP_PIXELS = 4.0         # default radius: this many crop pixels, in photo pixels


def gaussian_weights(sigma):
    """The kernel scipy.ndimage.gaussian_filter1d correlates with for order 0: radius int(4 sigma + 0.5), exp(-x^2 / (2 sigma^2))
    normalised by its sum.  -> (float64 [2 radius + 1], radius)."""
    sigma = float(sigma)
    radius = int(GAUSS_TRUNCATE * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def quad_coefficients(quad_corners, size):
    """The 8 numbers Image.transform(size, QUAD, corners) hands to Pillow's bilinear-quad map: corners in the order NW, SW, SE, NE
    (x, y), a (size x size) output.  x_src = a0 + a1 x + a2 y + a3 x y, y_src = a4 + a5 x + a6 y + a7 x y at pixel centres."""
    (nwx, nwy), (swx, swy), (sex, sey), (nex, ney) = [(float(p[0]), float(p[1])) for p in np.asarray(quad_corners).reshape(4, 2)]
    inv_w = inv_h = 1.0 / size
    return np.array([nwx, (nex - nwx) * inv_w, (swx - nwx) * inv_h, (sex - swx - nex + nwx) * inv_w * inv_h,
                     nwy, (ney - nwy) * inv_w, (swy - nwy) * inv_h, (sey - swy - ney + nwy) * inv_w * inv_h], np.float64)


def perspective_matrix(src4, dst4, exact=False):
    """The 3x3 homography that maps four source points onto four target points (what cv2.getPerspectiveTransform solves), by
    numpy's solve of the 8x8 system; both inputs pass through float32 like cv2's arguments (exact=True: they stay float64)."""
    s = (np.asarray(src4, np.float64) if exact else np.asarray(src4, np.float32).astype(np.float64)).reshape(4, 2)
    d = (np.asarray(dst4, np.float64) if exact else np.asarray(dst4, np.float32).astype(np.float64)).reshape(4, 2)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y, u, v = s[i, 0], s[i, 1], d[i, 0], d[i, 1]
        A[i] = (x, y, 1, 0, 0, 0, -x * u, -y * u)
        A[i + 4] = (0, 0, 0, x, y, 1, -x * v, -y * v)
        b[i], b[i + 4] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def align_plan(lm_68, height, width, output_size, transform_size=4096, enable_padding=True):
    """Geometry of one alignment.  lm_68: [68,2] (or more rows; the first 68 count) landmark pixels (x, y) of a height x width
    photo.  Returns a dict:
      quad float64 [4,2] (in the frame of the image the transform reads: after shrink, crop and pad), qsize,
      shrink (int; > 1 means the photo is first Lanczos-resized to `resized` = (w, h)), resized,
      crop (x0, y0, x1, y1) in the resized photo and `cropped` (whether it is a sub-window), border,
      pad (left, top, right, bottom) and `padded` (whether the padding branch runs), blur (sigma) with gauss_w / gauss_radius,
      coef float64 [8] (Pillow's quad coefficients of quad + 0.5), landmarks int32 [68,2] in the aligned image,
      image_size (w, h) of the image the transform reads, transform_size, output_size."""
    lm = np.asarray(lm_68, np.float64)
    if lm.ndim != 2 or lm.shape[0] < 68 or lm.shape[1] != 2:
        raise ValueError(f'landmarks must be [68,2] (or [81,2]) pixel coordinates, got {lm.shape}')
    lm = lm[:68]
    if not np.isfinite(lm).all():
        raise ValueError('landmarks are not finite')
    height, width, S, T = int(height), int(width), int(output_size), int(transform_size)
    if height < 1 or width < 1 or S < 1 or T < S or T > MAX_TRANSFORM:
        raise ValueError(f'need a non-empty photo and 1 <= output_size <= transform_size <= {MAX_TRANSFORM}')

    # the oriented square: eye line and eye-to-mouth line give its x axis, centre a little below the eyes
    eye_l, eye_r = np.mean(lm[36:42], axis=0), np.mean(lm[42:48], axis=0)
    eye_mid = (eye_l + eye_r) * 0.5
    eye_vec = eye_r - eye_l
    mouth_mid = (lm[48] + lm[54]) * 0.5
    down = mouth_mid - eye_mid
    ax = eye_vec - np.flipud(down) * [-1, 1]
    ax /= np.hypot(*ax)
    ax *= max(np.hypot(*eye_vec) * 2.0, np.hypot(*down) * 1.8)
    ay = np.flipud(ax) * [-1, 1]
    centre = eye_mid + down * 0.1
    quad = np.stack([centre - ax - ay, centre - ax + ay, centre + ax + ay, centre + ax - ay])
    qsize = np.hypot(*ax) * 2
    pts = lm
    w, h = width, height

    shrink = int(np.floor(qsize / S * 0.5))
    if shrink > 1:
        w, h = int(np.rint(float(width) / shrink)), int(np.rint(float(height) / shrink))
        quad /= shrink
        qsize /= shrink
        pts = pts / shrink
    resized = (w, h)

    def bbox(q):
        return (int(np.floor(min(q[:, 0]))), int(np.floor(min(q[:, 1]))), int(np.ceil(max(q[:, 0]))), int(np.ceil(max(q[:, 1]))))

    border = max(int(np.rint(qsize * 0.1)), 3)
    bx = bbox(quad)
    crop = (max(bx[0] - border, 0), max(bx[1] - border, 0), min(bx[2] + border, w), min(bx[3] + border, h))
    cropped = crop[2] - crop[0] < w or crop[3] - crop[1] < h
    if cropped:
        if crop[2] <= crop[0] or crop[3] <= crop[1]:
            raise ValueError('the face lies outside the photo')
        quad -= crop[0:2]
        pts = pts - np.array([crop[0], crop[1]])
        w, h = crop[2] - crop[0], crop[3] - crop[1]
    else:
        crop = (0, 0, w, h)

    bx = bbox(quad)
    pad = (max(-bx[0] + border, 0), max(-bx[1] + border, 0), max(bx[2] - w + border, 0), max(bx[3] - h + border, 0))
    padded = bool(enable_padding and max(pad) > border - 4)
    blur = qsize * 0.02
    gauss_w, gauss_radius = None, 0
    if padded:
        pad = tuple(int(v) for v in np.maximum(pad, int(np.rint(qsize * 0.3))))
        pts = pts + np.array([pad[0], pad[1]])
        quad += pad[:2]
        w, h = w + pad[0] + pad[2], h + pad[1] + pad[3]
        gauss_w, gauss_radius = gaussian_weights(blur)
    else:
        pad = (0, 0, 0, 0)

    corners = quad + 0.5
    M = perspective_matrix(corners, [[0, 0], [0, 1], [1, 1], [1, 0]])
    hom = M @ np.concatenate([pts, np.ones([pts.shape[0], 1])], axis=1).T
    out_pts = (hom[:2, :] / hom[2] * S).T
    return {'quad': quad, 'qsize': float(qsize), 'shrink': shrink, 'resized': resized, 'crop': crop, 'cropped': bool(cropped),
            'border': border, 'pad': pad, 'padded': padded, 'blur': float(blur), 'gauss_w': gauss_w, 'gauss_radius': gauss_radius,
            'coef': quad_coefficients(corners, T), 'landmarks': (out_pts + 0.5).astype('int32'), 'image_size': (w, h),
            'transform_size': T, 'output_size': S}


def pack_plan(plan):
    """The plan as ch_face_align takes it: float64 [CH_ALIGN_PLAN_LEN] (include/ctrlhair_hip.h)."""
    v = np.zeros(PLAN_LEN, np.float64)
    v[0] = plan['shrink']
    v[1:3] = plan['resized']
    v[3:7] = plan['crop']
    v[7] = 1.0 if plan['padded'] else 0.0
    v[8:12] = plan['pad']
    v[12:20] = plan['coef']
    v[20], v[21] = plan['transform_size'], plan['output_size']
    return v


def unalign_plan(plan, height, width):
    """The way back from an alignment: geometry that pastes an edited S x S crop of `plan` (align_plan's dict) into the height x width
    photo it was aligned from.  Coordinates are continuous with pixel i covering [i, i + 1).  A crop point (x, y) lies at
    NW + (x / S)(NE - NW) + (y / S)(SW - NW) of the frame the transform read (corners = quad + 0.5), the frame is the resized photo
    shifted by crop[:2] - pad[:2], and the Lanczos shrink maps edge to edge: photo = resized * (width / resized_w, height / resized_h).
    Returns a dict: A float64 [2,3] (photo pixel centre (X + 0.5, Y + 0.5, 1) -> (x, y)), Ainv [2,3] (the inverse), bbox (x0, y0, x1, y1)
    of the quad in the photo, clipped to it, scale (crop pixels per photo pixel), output_size."""
    height, width, S = int(height), int(width), int(plan['output_size'])
    corners = np.asarray(plan['quad'], np.float64) + 0.5
    Hm = perspective_matrix([[0, 0], [0, S], [S, S], [S, 0]], corners, exact=True)           # crop -> frame
    if np.abs(Hm[2] - [0.0, 0.0, 1.0]).max() > 1e-9:
        raise ValueError('the quad of the plan is not a parallelogram: the crop-to-photo map is not affine')
    rw, rh = plan['resized']
    if plan['shrink'] <= 1 and (rw, rh) != (width, height):
        raise ValueError(f'the plan was made for a {rw} x {rh} photo, not {width} x {height}')
    if plan['shrink'] > 1 and (rw, rh) != (int(np.rint(float(width) / plan['shrink'])), int(np.rint(float(height) / plan['shrink']))):
        raise ValueError(f'the plan (shrink {plan["shrink"]}, resized {rw} x {rh}) was not made for a {width} x {height} photo')
    shift = np.asarray(plan['crop'][:2], np.float64) - np.asarray(plan['pad'][:2], np.float64)
    zoom = np.array([width / rw, height / rh])
    Ainv = np.empty((2, 3))
    Ainv[:, :2] = Hm[:2, :2] * zoom[:, None]
    Ainv[:, 2] = (Hm[:2, 2] + shift) * zoom
    L = np.linalg.inv(Ainv[:, :2])
    A = np.concatenate([L, -(L @ Ainv[:, 2])[:, None]], axis=1)
    scale = float(max(np.hypot(*A[:, 0]), np.hypot(*A[:, 1])))
    if scale > UNALIGN_MAX_SCALE:
        raise ValueError(f'the crop has {scale:.1f} pixels per photo pixel; paste-back supports at most {UNALIGN_MAX_SCALE}')
    q = (Ainv[:, :2] @ np.array([[0, 0, S, S], [0, S, S, 0]], np.float64) + Ainv[:, 2:3]).T          # the quad in the photo
    bbox = (max(int(np.floor(q[:, 0].min())), 0), max(int(np.floor(q[:, 1].min())), 0),
            min(int(np.ceil(q[:, 0].max())), width), min(int(np.ceil(q[:, 1].max())), height))
    if bbox[2] <= bbox[0] or bbox[3] <= bbox[1]:
        raise ValueError('the face lies outside the photo: nothing to paste')
    return {'A': A, 'Ainv': Ainv, 'bbox': bbox, 'scale': scale, 'output_size': S}


def pack_unalign(plan_u):
    """unalign_plan's dict as ch_face_unalign takes it: float64 [CH_UNALIGN_PLAN_LEN] (include/ctrlhair_hip.h)."""
    v = np.zeros(UNALIGN_PLAN_LEN, np.float64)
    v[0:6] = np.asarray(plan_u['A'], np.float64).reshape(6)
    v[6:10] = plan_u['bbox']
    v[10], v[11] = plan_u['scale'], plan_u['output_size']
    return v


def matte_params(matte, scale):
    """(radius, eps) of the guided-filter matte of paste_back (ch_face_unalign_matte).  matte: True, or a dict with 'radius' (photo
    pixels) and / or 'eps' (regularisation, in units of a guide scaled to [0, 1]); scale: crop pixels per photo pixel (unalign_plan's
    'scale').  Defaults: radius min(64, max(1, ceil(4 / scale))) photo pixels -- four crop pixels of label uncertainty -- and eps
    1e-4.  Both defaults are design choices with no measurement behind them: nothing here has compared mattes on real photos.
    Raises ValueError for a radius outside [1, 64] or an eps that is not positive and finite."""
    if matte is True:
        matte = {}
    if not isinstance(matte, dict):
        raise ValueError(f'matte must be True or a dict with radius and / or eps, got {matte!r}')
    unknown = set(matte) - {'radius', 'eps'}
    if unknown:
        raise ValueError(f'matte: unknown keys {sorted(unknown)} (radius, eps)')
    scale = float(scale)
    if not scale > 0 or not np.isfinite(scale):
        raise ValueError(f'scale must be positive, got {scale}')
    radius = matte.get('radius')
    if radius is None:
        radius = min(MATTE_MAX_RADIUS, max(1, int(np.ceil(MATTE_CROP_PIXELS / scale))))
    if int(radius) != radius or not 1 <= int(radius) <= MATTE_MAX_RADIUS:
        raise ValueError(f'matte radius must be an integer in [1, {MATTE_MAX_RADIUS}] photo pixels, got {radius!r}')
    eps = matte.get('eps')
    eps = MATTE_DEFAULT_EPS if eps is None else float(eps)
    if not eps > 0 or not np.isfinite(eps):
        raise ValueError(f'matte eps must be positive and finite, got {eps!r}')
    return int(radius), eps


def read_photo(path, orient=True, reader=None):
    """A photo file for FaceAligner.align / HairEditor.crop_face: (pixels uint8 [H,W,3], (orientation, exif bytes or None, icc profile or
    None)).  orient: the pixels are made upright by the file's EXIF orientation, as viewers and landmark detectors see them, and the
    EXIF block comes without the tag; landmarks found on the stored pixels move along with orient.orient_points.  reader: None -- Pillow
    reads the file, the pixels are numpy; a device reader (dataset._PhotoReader) -- it is decoded and turned on the device, the pixels
    are a device tensor, the same bytes."""
    from . import dataset
    read = dataset.read_rgb if reader is None else reader.read_rgb
    return read(path, orient=bool(orient), metadata=True)


class FaceAligner(DeviceOp):
    """recreate_aligned_images on the device.  Attached to HipModels as `aligner`; also usable alone (no network weights)."""

    def _u8(self, a, channels=None):
        import torch
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
            a = torch.from_numpy(a if a.flags.writeable else a.copy())       # arrays of PIL images are read-only
        t = a
        if t.dtype != torch.uint8:
            raise TypeError(f'expected a uint8 image, got {t.dtype}')
        t = t.to(self.device).contiguous()
        if t.dim() != 3 or (channels is not None and t.shape[2] != channels):
            raise ValueError(f'expected an [H,W,{channels or "C"}] image, got {tuple(t.shape)}')
        return t

    @staticmethod
    def _f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(C.c_void_p)

    # ---- stages ------------------------------------------------------------------------------------------------------------
    def resample(self, img, size):
        """Image.resize(size, LANCZOS) of a uint8 [H,W,C] image (1 <= C <= 4); size = (width, height) -> uint8 [h,w,C] tensor."""
        import torch
        x = self._u8(img)
        Hs, Ws, Cn = (int(v) for v in x.shape)
        Wd, Hd = int(size[0]), int(size[1])
        if Wd < 1 or Hd < 1:
            raise ValueError(f'empty target size {size}')
        out = torch.empty(Hd, Wd, Cn, dtype=torch.uint8, device=self.device)
        need = int(self.handle.lib.ch_resample_lanczos_workspace_bytes(Hs, Ws, Cn, Hd, Wd))
        ws = self._buffer('_ws',need)
        self.handle.call('ch_resample_lanczos_u8', x.data_ptr(), Hs, Ws, Cn, out.data_ptr(), Hd, Wd, ws.data_ptr(), ws.numel(),
                         self._stream())
        return out

    def quad_warp(self, img, corners, transform_size, output_size):
        """Image.transform((T, T), QUAD, corners.flatten(), BILINEAR) then resize((S, S), LANCZOS) when S < T.  corners [4,2]:
        NW, SW, SE, NE.  -> uint8 [S,S,3] tensor."""
        import torch
        x = self._u8(img, 3)
        T, S = int(transform_size), int(output_size)
        coef, cp = self._f64(quad_coefficients(corners, T))
        out = torch.empty(S, S, 3, dtype=torch.uint8, device=self.device)
        ws = self._buffer('_ws',int(self.handle.lib.ch_quad_warp_workspace_bytes(T, S)))
        self.handle.call('ch_quad_warp_resample_u8', x.data_ptr(), int(x.shape[0]), int(x.shape[1]), cp, T, S, out.data_ptr(),
                         ws.data_ptr(), ws.numel(), self._stream())
        return out

    def pad_feather(self, img, pad, blur):
        """crop.py:83-92: reflect pad by (left, top, right, bottom), Gaussian feather with sigma `blur`, median fill.  -> uint8
        [H+top+bottom, W+left+right, 3] tensor."""
        import torch
        x = self._u8(img, 3)
        Hs, Ws = int(x.shape[0]), int(x.shape[1])
        pads = np.ascontiguousarray(pad, dtype=np.int32).reshape(4)
        w, radius = gaussian_weights(blur)
        w, wp = self._f64(w)
        pp = pads.ctypes.data_as(C.c_void_p)
        if pads.min() < 1:
            raise ValueError(f'pad widths must be >= 1, got {tuple(pads)}')
        out = torch.empty(Hs + int(pads[1]) + int(pads[3]), Ws + int(pads[0]) + int(pads[2]), 3, dtype=torch.uint8, device=self.device)
        ws = self._buffer('_ws',int(self.handle.lib.ch_align_pad_workspace_bytes(Hs, Ws, pp, radius)))
        self.handle.call('ch_align_pad_feather_u8', x.data_ptr(), Hs, Ws, pp, wp, radius, out.data_ptr(), ws.data_ptr(), ws.numel(),
                         self._stream())
        return out

    # ---- the whole alignment -------------------------------------------------------------------------------------------------
    def run_plan(self, img, plan):
        """One ch_face_align call for a plan of align_plan -> uint8 [S,S,3] tensor."""
        import torch
        x = self._u8(img, 3)
        H, W = int(x.shape[0]), int(x.shape[1])
        S = int(plan['output_size'])
        pv, pp = self._f64(pack_plan(plan))
        radius = int(plan['gauss_radius'])
        gw, gp = (self._f64(plan['gauss_w']) if plan['padded'] else (None, None))
        need = int(self.handle.lib.ch_face_align_workspace_bytes(H, W, pp, radius))
        if need == 0:
            raise ValueError('the plan does not fit the photo (see ch_face_align in include/ctrlhair_hip.h)')
        ws = self._buffer('_ws',need)
        out = torch.empty(S, S, 3, dtype=torch.uint8, device=self.device)
        self.handle.call('ch_face_align', x.data_ptr(), H, W, pp, gp, radius, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        return out

    def align(self, img_rgb_u8, lm_68, output_size, transform_size=4096, enable_padding=True, return_plan=False):
        """recreate_aligned_images(img, lm_68, output_size): img uint8 [H,W,3] RGB (numpy is uploaded), lm_68 [68,2] pixels ->
        (aligned uint8 [S,S,3] device tensor, int32 [68,2] landmarks in it); return_plan=True -> (aligned, align_plan's dict), what
        paste_back needs to put an edit of the crop back into the photo."""
        shape = tuple(img_rgb_u8.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f'expected an RGB image [H,W,3], got {shape}')
        plan = align_plan(lm_68, shape[0], shape[1], output_size, transform_size, enable_padding)
        if return_plan:
            return self.run_plan(img_rgb_u8, plan), plan
        return self.run_plan(img_rgb_u8, plan), plan['landmarks']

    def paste_back(self, photo, edits, plan, weight=None, feather=None, matte=None, return_alpha=False):
        """The way back: composite edited crops into the photo they were aligned from, ONE ch_face_unalign call for all of them.
        photo uint8 [H,W,3]; edits uint8 [S,S,3] or [N,S,S,3] (numpy is uploaded); plan: align_plan's dict (align(...,
        return_plan=True)) or unalign_plan's; weight: optional uint8 [S,S] map, 255 = the edit, 0 = the photo; feather: width in crop
        pixels of the ramp at the crop's border (default S / 16, <= 0 = hard edge).  -> uint8 [N,H,W,3] device tensor.
        matte (True or a dict, see matte_params): the weight map, sampled nearest, is refined by a guided filter whose guide is the
        photo (ONE ch_face_unalign_matte call), so the pasted region follows the photo's edges; needs `weight`.  return_alpha=True
        (with matte) -> (out, alpha float32 [bh,bw] over the plan's bbox)."""
        import torch
        if matte is None and return_alpha:
            raise ValueError('return_alpha needs matte (the plain paste-back keeps no alpha plane)')
        if matte is not None and weight is None:
            raise ValueError('matte refines a weight map: pass weight=')
        x = self._u8(photo, 3)
        H, W = int(x.shape[0]), int(x.shape[1])
        pu = plan if 'A' in plan else unalign_plan(plan, H, W)
        S = int(pu['output_size'])
        e = edits if isinstance(edits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(edits, dtype=np.uint8)))
        if e.dtype != torch.uint8:
            raise TypeError(f'expected uint8 edits, got {e.dtype}')
        if e.dim() == 3:
            e = e[None]
        if e.dim() != 4 or tuple(e.shape[1:]) != (S, S, 3) or e.shape[0] < 1:
            raise ValueError(f'expected edits [N,{S},{S},3] (the plan\'s output_size is {S}), got {tuple(e.shape)}')
        e = e.to(self.device).contiguous()
        wp = None
        if weight is not None:
            w = weight if isinstance(weight, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(weight, dtype=np.uint8)))
            if w.dtype != torch.uint8 or tuple(w.shape) != (S, S):
                raise ValueError(f'expected a uint8 weight map [{S},{S}], got {w.dtype} {tuple(w.shape)}')
            w = w.to(self.device).contiguous()
            wp = w.data_ptr()
        bx = pu['bbox']
        if pu['scale'] > UNALIGN_MAX_SCALE or bx[0] < 0 or bx[1] < 0 or bx[2] > W or bx[3] > H or bx[2] <= bx[0] or bx[3] <= bx[1]:
            raise ValueError(f'the plan (bbox {tuple(bx)}, scale {pu["scale"]:.2f}) does not fit a {W} x {H} photo')
        N = int(e.shape[0])
        pv, pp = self._f64(pack_unalign(pu))
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=self.device)
        feather = float(S / 16.0 if feather is None else feather)
        if matte is None:
            self.handle.call('ch_face_unalign', x.data_ptr(), H, W, e.data_ptr(), N, wp, pp, feather, out.data_ptr(), self._stream())
            return out
        radius, eps = matte_params(matte, pu['scale'])
        need = int(self.handle.lib.ch_face_unalign_matte_workspace_bytes(H, W, pp, radius))
        if need == 0:
            raise ValueError('the plan does not fit the photo (see ch_face_unalign_matte in include/ctrlhair_hip.h)')
        ws = self._buffer('_ws',need)
        alpha = torch.empty(bx[3] - bx[1], bx[2] - bx[0], dtype=torch.float32, device=self.device) if return_alpha else None
        self.handle.call('ch_face_unalign_matte', x.data_ptr(), H, W, e.data_ptr(), N, wp, pp, feather, radius, eps, out.data_ptr(),
                         None if alpha is None else alpha.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        return (out, alpha) if return_alpha else out
