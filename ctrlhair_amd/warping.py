"""Hair-shape transfer: the mask warp of wrap_codes/mask_adaptor.py:87-143 (`hair_mask_transfer_wrap`) on the HIP library.

The reference writes node files, runs Shewchuk's *Triangle* (-q30) and a libigl ARAP binary through os.system, rasterises the
deformed mesh with a Cython module and samples the padded hair mask with cv2.remap.  Here the mesh is built on the host
(`build_nodes`, `build_mesh`: scipy Delaunay over the reference's 273 constrained nodes plus a fixed lattice of free interior
points) and everything after it -- ARAP solve, UV render, edge fix, sampling, crop, naive_transfer -- is ONE call of
`ch_mask_warp_batch` for B pairs (csrc/mask_warp.hip).  No CPU fallback: without the library / a GPU `MaskWarper` raises.
With mesher='device' only the points are made on the host (`build_points_batch`, numpy over the batch): one upload, then
`ch_delaunay_batch` (csrc/delaunay.hip) triangulates all B point sets in one launch and `ch_mask_warp_batch_dev` reads the
descriptors from device memory, so the call never synchronises.  The two meshers may pick different diagonals inside
co-circular quads of the lattice; 'host' stays the default.

Differences from the reference, all stated: (1) the mesh is not Triangle's, so the warp is not pixel-identical to the reference's
(`warp_with_mesh` takes any mesh, e.g. Triangle's own); (2) my_arap writes U and V / (W - 1) to an .obj with 6 significant digits
before the rasteriser reads them -- here they stay float32; (3) cv2 is not a dependency: the sampling step restates OpenCV's
documented remap arithmetic (coordinates rounded to 1/32 px with cvRound, bilinear tap weights that are multiples of 1/1024,
constant border 0) and is unpinned against cv2 itself, like the OpenCV glue of hostutil.py.  With a 0/1 image and the
reference's .astype('uint8') truncation that arithmetic reduces to: a pixel is hair iff every tap with non-zero weight is hair.
"""
import ctypes as C

import numpy as np

from .devop import DeviceOp

HAIR_IDX = 13
IMG = 512                       # the warp is defined on 512 x 512 parsings (mask_adaptor.py:121-122)
BG_WIDTH = 80                   # mask_adaptor.py:119
CANVAS = IMG + 2 * BG_WIDTH     # 672
NUM_FRAME = 50                  # triangle_wrap_hair.py:53 numPoints
DROPPED_LANDMARKS = (17, 19, 25, 26)            # mask_adaptor.py:110
CHOSEN_LANDMARKS = [k for k in range(81) if k not in DROPPED_LANDMARKS]
N_CONSTRAINED = len(CHOSEN_LANDMARKS) + 4 * NUM_FRAME - 4      # 77 + 196
LATTICE_STEP = 2                # free lattice points on every 2nd frame coordinate (27.4 px): see DESIGN.md, "Mask warp"
MAX_V, MAX_F = 2048, 4096       # CH_WARP_MAX_V / CH_WARP_MAX_F


def build_nodes(hair_lm_81, face_lm_81):
    """step_3/generate_node.py:23-72 on the canvas of mask_adaptor.py:105-131.  hair_lm_81 (donor of the shape), face_lm_81:
    float [81,2] in [0,1] -> (nodes float64 [273,2], targets float64 [273,2]): the 77 kept donor landmarks constrained to the 77
    face landmarks, then the frame of the 672 x 672 canvas (top, bottom, left, right) constrained to itself.  The reference
    prints frame nodes with 4 decimals and everything else with 8; so do the values here."""
    hl = np.asarray(hair_lm_81, np.float64).reshape(81, 2)[CHOSEN_LANDMARKS] * IMG + BG_WIDTH
    fl = np.asarray(face_lm_81, np.float64).reshape(81, 2)[CHOSEN_LANDMARKS] * IMG + BG_WIDTH
    r = np.linspace(0, CANVAS - 1, NUM_FRAME)
    lo, hi = np.zeros(NUM_FRAME), np.full(NUM_FRAME, CANVAS - 1.0)
    frame = np.concatenate([np.stack([r, lo], 1), np.stack([r, hi], 1),
                            np.stack([lo[1:-1], r[1:-1]], 1), np.stack([hi[1:-1], r[1:-1]], 1)])
    nodes = np.concatenate([np.round(hl, 8), np.round(frame, 4)])
    targets = np.concatenate([np.round(fl, 8), np.round(frame, 8)])
    return nodes, targets


def build_mesh(nodes, lattice_step=LATTICE_STEP):
    """Triangulation of the constrained nodes plus free interior points (the role of `triangle -q30`'s Steiner points): a square
    lattice on every `lattice_step`-th frame coordinate, minus the points closer than half a lattice step to a landmark, Delaunay
    (scipy / Qhull).  -> (V float32 [n,2] with V[:273] = nodes, F int32 [m,3] counter-clockwise in (x, y), sorted rows,
    b int32 [273] = arange(273)).  Deterministic for given nodes."""
    from scipy.spatial import Delaunay
    nodes = np.asarray(nodes, np.float64)
    if nodes.shape != (N_CONSTRAINED, 2):
        raise ValueError(f'nodes must be [{N_CONSTRAINED},2] (build_nodes), got {nodes.shape}')
    r = np.linspace(0, CANVAS - 1, NUM_FRAME)[1:-1:lattice_step]
    gx, gy = np.meshgrid(r, r)
    lat = np.stack([gx.ravel(), gy.ravel()], 1)
    lm = nodes[:len(CHOSEN_LANDMARKS)]
    step = (CANVAS - 1) / (NUM_FRAME - 1) * lattice_step
    d2 = ((lat[:, None, :] - lm[None, :, :]) ** 2).sum(-1).min(1)
    lat = lat[d2 >= (0.5 * step) ** 2]
    V = np.concatenate([nodes, lat]).astype(np.float32)
    F = Delaunay(V.astype(np.float64)).simplices.astype(np.int64)
    a, b, c = V[F[:, 0]].astype(np.float64), V[F[:, 1]].astype(np.float64), V[F[:, 2]].astype(np.float64)
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    F = F[area2 != 0]
    area2 = area2[area2 != 0]
    F[area2 < 0] = F[area2 < 0][:, [0, 2, 1]]
    # rotate each row so that its smallest index comes first (keeps the orientation), then sort the rows
    k = F.argmin(1)
    F = np.stack([F[np.arange(len(F)), (k + j) % 3] for j in range(3)], 1)
    F = F[np.lexsort((F[:, 2], F[:, 1], F[:, 0]))]
    check_mesh(V, F, np.arange(N_CONSTRAINED))
    return V, F.astype(np.int32), np.arange(N_CONSTRAINED, dtype=np.int32)


GRID = 1 << 20                  # exactness domain of ch_delaunay_batch: float32 multiples of 2^-20 in [0, 1024)
DOMAIN_END = 1024.0


def _lattice():
    r = np.linspace(0, CANVAS - 1, NUM_FRAME)[1:-1:LATTICE_STEP]
    gx, gy = np.meshgrid(r, r)
    return np.stack([gx.ravel(), gy.ravel()], 1), (CANVAS - 1) / (NUM_FRAME - 1) * LATTICE_STEP


def build_points_batch(hair_lm, face_lm):
    """build_nodes plus the lattice filter of build_mesh for B pairs at once (numpy over the batch, no triangulation).
    hair_lm, face_lm: float [B,81,2] in [0,1] -> (V float32 [sum n,2] packed, counts int32 [B], targets float32 [B,273,2]).
    The rows of pair i are bit-identical to build_mesh(build_nodes(hair_lm[i], face_lm[i])[0])[0]; its constrained vertices are
    its first 273 rows.  Raises ValueError naming the pair for a coordinate outside the exactness domain of ch_delaunay_batch
    (finite float32 multiples of 2^-20 in [0, 1024)) and for a duplicate point."""
    hl = np.asarray(hair_lm, np.float64).reshape(-1, 81, 2)
    fl = np.asarray(face_lm, np.float64).reshape(-1, 81, 2)
    if len(hl) != len(fl) or len(hl) < 1:
        raise ValueError('one landmark set per image on both sides')
    B = len(hl)
    r = np.linspace(0, CANVAS - 1, NUM_FRAME)
    lo, hi = np.zeros(NUM_FRAME), np.full(NUM_FRAME, CANVAS - 1.0)
    frame = np.concatenate([np.stack([r, lo], 1), np.stack([r, hi], 1),
                            np.stack([lo[1:-1], r[1:-1]], 1), np.stack([hi[1:-1], r[1:-1]], 1)])
    lm = np.round(hl[:, CHOSEN_LANDMARKS] * IMG + BG_WIDTH, 8)                                  # [B,77,2]
    nodes = np.concatenate([lm, np.broadcast_to(np.round(frame, 4), (B,) + frame.shape)], 1)    # [B,273,2]
    targets = np.concatenate([np.round(fl[:, CHOSEN_LANDMARKS] * IMG + BG_WIDTH, 8),
                              np.broadcast_to(np.round(frame, 8), (B,) + frame.shape)], 1)
    lat, step = _lattice()
    keep = np.empty((B, len(lat)), bool)
    for i0 in range(0, B, 64):           # the float64 distance test of build_mesh, 64 pairs at a time (45 MB)
        d2 = ((lat[None, :, None, :] - lm[i0:i0 + 64, None, :, :]) ** 2).sum(-1).min(2)
        keep[i0:i0 + 64] = d2 >= (0.5 * step) ** 2
    lat32 = lat.astype(np.float32)
    nodes32 = nodes.astype(np.float32)
    counts = (N_CONSTRAINED + keep.sum(1)).astype(np.int32)
    V = np.empty((int(counts.sum()), 2), np.float32)
    o = 0
    for i in range(B):
        n = int(counts[i])
        Vi = V[o:o + n]
        Vi[:N_CONSTRAINED] = nodes32[i]
        Vi[N_CONSTRAINED:] = lat32[keep[i]]
        g = Vi.astype(np.float64) * GRID
        if not (np.isfinite(g).all() and (g >= 0).all() and (g < DOMAIN_END * GRID).all() and (g == np.rint(g)).all()):
            raise ValueError(f'pair {i}: a mesh point is outside the exactness domain of the device mesher (float32 multiples of '
                             f'2^-20 in [0, 1024)); landmarks must lie inside the 672 x 672 canvas')
        key = g[:, 0].astype(np.int64) << 30 | g[:, 1].astype(np.int64)
        if len(np.unique(key)) != n:
            raise ValueError(f'pair {i}: duplicate mesh point (two landmarks coincide, or a landmark sits on a frame node)')
        o += n
    return V, counts, targets.astype(np.float32)


def check_mesh(V, F, b):
    """What ch_mask_warp_batch supports: sizes within CH_WARP_MAX_V / CH_WARP_MAX_F, indices in range.  Raises ValueError."""
    V, F, b = np.asarray(V), np.asarray(F), np.asarray(b)
    if V.ndim != 2 or V.shape[1] != 2 or F.ndim != 2 or F.shape[1] != 3:
        raise ValueError(f'mesh must be V [n,2], F [m,3]; got {V.shape}, {F.shape}')
    if not (3 <= len(V) <= MAX_V and 1 <= len(F) <= MAX_F):
        raise ValueError(f'mesh has {len(V)} vertices / {len(F)} triangles; the GPU solver holds one mesh in LDS and supports '
                         f'3..{MAX_V} vertices and 1..{MAX_F} triangles')
    if F.min() < 0 or F.max() >= len(V) or (len(b) and (b.min() < 0 or b.max() >= len(V))):
        raise ValueError('mesh index out of range')
    if not np.isfinite(V).all():
        raise ValueError('mesh has non-finite vertices')


class MaskWarper(DeviceOp):
    """The built-in warper of Backend.transfer_latent_representation('shape') and EditPipeline.transfer_shape."""

    def __init__(self, handle=None, device=None):
        super().__init__(handle, device)
        self.last_mesh_status = self.last_mesh = None     # of the last warp_batch(mesher='device')

    # ---- the ABI call ---------------------------------------------------------------------------------------------------
    def _labels(self, a, B):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8)))
        t = t.to(self.device).to(torch.uint8).reshape(-1, IMG, IMG)
        if t.shape[0] != B:
            raise ValueError(f'expected {B} label maps of {IMG}x{IMG}, got {tuple(t.shape)}')
        return t.contiguous()

    def warp_meshes(self, hair_labels, face_labels, meshes, U=None, return_uv=False, return_U=False):
        """B pairs with explicit meshes in one ch_mask_warp_batch call.  hair_labels, face_labels: uint8 [B,512,512] (numpy or
        torch, any device); meshes: list of B tuples (V [n,2], F [m,3], b [k], bc [k,2]) in canvas coordinates; U: optional list
        of deformed positions [n,2] per pair (then the ARAP solve is skipped).  -> labels uint8 [B,512,512] on the device, or a
        dict {'labels', 'uv' [B,672,672,2], 'U' list of [n,2] tensors} when return_uv / return_U is set."""
        import torch
        B = len(meshes)
        if B < 1:
            raise ValueError('no pairs')
        hair, face = self._labels(hair_labels, B), self._labels(face_labels, B)
        desc = np.zeros((B, 6), np.int32)
        vo = fo = bo = 0
        Vs, Fs, bs, bcs = [], [], [], []
        for i, (V, F, b, bc) in enumerate(meshes):
            V, F = np.asarray(V, np.float32), np.asarray(F, np.int32)
            b, bc = np.asarray(b, np.int32).reshape(-1), np.asarray(bc, np.float32).reshape(-1, 2)
            check_mesh(V, F, b)
            if len(b) != len(bc):
                raise ValueError(f'pair {i}: {len(b)} constrained indices but {len(bc)} targets')
            desc[i] = (vo, len(V), fo, len(F), bo, len(b))
            vo, fo, bo = vo + len(V), fo + len(F), bo + len(b)
            Vs.append(V), Fs.append(F), bs.append(b), bcs.append(bc)
        dev = self.device
        Vd = torch.from_numpy(np.concatenate(Vs)).to(dev)
        Fd = torch.from_numpy(np.concatenate(Fs)).to(dev)
        bd = torch.from_numpy(np.concatenate(bs + [np.zeros(1, np.int32)])).to(dev)
        bcd = torch.from_numpy(np.concatenate(bcs + [np.zeros((1, 2), np.float32)])).to(dev)
        Uin = None
        if U is not None:
            Uin = np.concatenate([np.asarray(u, np.float32).reshape(-1, 2) for u in U])
            if len(Uin) != vo:
                raise ValueError('U must give one position per mesh vertex')
            Uin = torch.from_numpy(Uin).to(dev)
        out = torch.empty(B, IMG, IMG, dtype=torch.uint8, device=dev)
        uv = torch.empty(B, CANVAS, CANVAS, 2, dtype=torch.float32, device=dev) if return_uv else None
        Uout = torch.empty(vo, 2, dtype=torch.float32, device=dev) if return_U else None
        ws = self._buffer('_ws', int(self.handle.lib.ch_mask_warp_workspace_bytes(B)))
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.handle.call('ch_mask_warp_batch', hair.data_ptr(), face.data_ptr(), Vd.data_ptr(), Fd.data_ptr(), bd.data_ptr(),
                         bcd.data_ptr(), desc.ctypes.data_as(C.c_void_p), ptr(Uin), out.data_ptr(), ptr(uv), ptr(Uout),
                         ws.data_ptr(), ws.numel(), B, self._stream())
        if not (return_uv or return_U):
            return out
        res = {'labels': out}
        if return_uv:
            res['uv'] = uv
        if return_U:
            res['U'] = list(torch.split(Uout, [int(n) for n in desc[:, 1]]))
        return res

    # ---- public entry points -------------------------------------------------------------------------------------------
    def warp_with_mesh(self, hair_parsing, face_parsing, V, F, b, bc, U=None, return_uv=False, return_U=False):
        """One pair on a given mesh (tests, or a mesher of your own such as Triangle).  -> labels uint8 [512,512] on the
        device, or the dict of warp_meshes with the batch dimension removed."""
        r = self.warp_meshes(np.asarray(hair_parsing)[None] if not hasattr(hair_parsing, 'to') else hair_parsing[None],
                             np.asarray(face_parsing)[None] if not hasattr(face_parsing, 'to') else face_parsing[None],
                             [(V, F, b, bc)], U=None if U is None else [U], return_uv=return_uv, return_U=return_U)
        if not isinstance(r, dict):
            return r[0]
        return {k: v[0] for k, v in r.items()}

    def _delaunay(self, Vd, counts):
        """ch_delaunay_batch on packed device points.  -> (F int32 [B,MAX_F,3], n_f int32 [B], status int32 [B]) on the device;
        the workspace (its counters included) stays in self._dws.  No synchronisation."""
        import torch
        B = len(counts)
        v_desc = np.zeros((B, 2), np.int32)
        v_desc[:, 1] = counts
        v_desc[1:, 0] = np.cumsum(counts)[:-1]
        F = torch.empty(B, MAX_F, 3, dtype=torch.int32, device=self.device)
        n_f = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        ws = self._buffer('_dws', int(self.handle.lib.ch_delaunay_workspace_bytes(B)))
        self.handle.call('ch_delaunay_batch', Vd.data_ptr(), v_desc.ctypes.data_as(C.c_void_p), F.data_ptr(), n_f.data_ptr(),
                         status.data_ptr(), ws.data_ptr(), ws.numel(), B, self._stream())
        return F, n_f, status

    def delaunay_counters(self, B):
        """Per set of the last ch_delaunay_batch call: int64 [B,2] = (incircle tests, those decided in integers).  Synchronises."""
        head = (B * 8 + 255) // 256 * 256
        return self._dws[head:head + 16 * B].cpu().numpy().view(np.uint64).reshape(B, 2).astype(np.int64)

    def triangulate(self, V_list):
        """Exact Delaunay triangulation of each point set of V_list (float [n,2] on the 2^-20 grid of [0, 1024), 3 <= n <= 2048)
        in ONE ch_delaunay_batch call.  -> list of (F int32 [m,3] in canonical form, status): status 0, or a CH_DELAUNAY_* code
        with an empty F.  Synchronises (the results are copied to the host)."""
        import torch
        Vs = [np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 2)) for V in V_list]
        if not Vs:
            raise ValueError('no point sets')
        counts = np.array([len(V) for V in Vs], np.int32)
        packed = np.concatenate(Vs) if counts.sum() else np.zeros((0, 2), np.float32)
        Vd = torch.from_numpy(np.concatenate([packed, np.zeros((1, 2), np.float32)])).to(self.device)
        F, n_f, status = self._delaunay(Vd, counts)
        F, n_f, status = F.cpu().numpy(), n_f.cpu().numpy(), status.cpu().numpy()
        return [(F[i, :int(n_f[i])].copy(), int(status[i])) for i in range(len(Vs))]

    def _warp_batch_device(self, hair_labels, face_labels, hl, fl):
        import torch
        V, counts, targets = build_points_batch(hl, fl)
        B, nV, nB = len(counts), len(V), N_CONSTRAINED
        hair, face = self._labels(hair_labels, B), self._labels(face_labels, B)
        desc = np.zeros((B, 6), np.int32)
        desc[1:, 0] = np.cumsum(counts)[:-1]
        desc[:, 1] = counts
        desc[:, 2] = np.arange(B) * MAX_F              # F is [B, MAX_F, 3]; column 3 (n_f) is filled on the device
        desc[:, 4] = np.arange(B) * nB
        desc[:, 5] = nB
        # one upload: V | bc | b | desc as 32-bit words
        words = np.concatenate([V.view(np.int32).ravel(), targets.view(np.int32).ravel(),
                                np.tile(np.arange(nB, dtype=np.int32), B), desc.ravel()])
        buf = torch.from_numpy(words).to(self.device)
        o1, o2, o3 = 2 * nV, 2 * nV + 2 * B * nB, 2 * nV + 3 * B * nB
        Vd, bcd, bd, descd = buf[:o1].view(torch.float32), buf[o1:o2].view(torch.float32), buf[o2:o3], buf[o3:].view(B, 6)
        F, n_f, status = self._delaunay(Vd, counts)
        descd[:, 3] = n_f                              # a failed set has n_f = 0: the warp refuses its descriptor, identity map
        out = torch.empty(B, IMG, IMG, dtype=torch.uint8, device=self.device)
        ws = self._buffer('_ws', int(self.handle.lib.ch_mask_warp_workspace_bytes(B)))
        self.handle.call('ch_mask_warp_batch_dev', hair.data_ptr(), face.data_ptr(), Vd.data_ptr(), F.data_ptr(), bd.data_ptr(),
                         bcd.data_ptr(), descd.data_ptr(), None, out.data_ptr(), None, None, ws.data_ptr(), ws.numel(), B,
                         self._stream())
        self.last_mesh_status = status
        self.last_mesh = {'V': Vd.view(-1, 2), 'counts': counts, 'F': F, 'n_f': n_f, 'bc': targets}
        return out

    def warp_batch(self, hair_labels, face_labels, hair_lm_81, face_lm_81, mesher='host'):
        """B pairs, one ABI call.  hair_labels (donors of the shape), face_labels: uint8 [B,512,512] device tensors (numpy is
        uploaded); hair_lm_81, face_lm_81: float [B,81,2] in [0,1] (host).  -> uint8 [B,512,512] on the device: warped hair 13,
        the face's own hair 255, else face_labels (naive_transfer).  Pair i is bit-identical to a call with that pair alone.
        mesher='host': scipy Delaunay per pair on the host, then ch_mask_warp_batch.  mesher='device': build_points_batch, one
        upload, ch_delaunay_batch, ch_mask_warp_batch_dev -- no synchronisation; the per-pair mesher statuses stay on the device
        in self.last_mesh_status (int32 [B], 0 = ok; a failed pair is warped with the identity map) and the meshes in
        self.last_mesh."""
        if mesher not in ('host', 'device'):
            raise ValueError(f"mesher must be 'host' or 'device', got {mesher!r}")
        hl, fl = np.asarray(hair_lm_81, np.float64).reshape(-1, 81, 2), np.asarray(face_lm_81, np.float64).reshape(-1, 81, 2)
        if len(hl) != len(fl):
            raise ValueError('one landmark set per image on both sides')
        if mesher == 'device':
            return self._warp_batch_device(hair_labels, face_labels, hl, fl)
        meshes = []
        for h, f in zip(hl, fl):
            nodes, targets = build_nodes(h, f)
            V, F, b = build_mesh(nodes)
            meshes.append((V, F, b, targets))
        return self.warp_meshes(hair_labels, face_labels, meshes)

    def warp(self, hair_parsing, face_parsing, hair_lm_81, face_lm_81, warp_temp_folder=None, mesher='host'):
        """Drop-in for hair_mask_transfer_wrap (mask_adaptor.py:87-143): numpy in, (result_parsing int [512,512],
        {'hair_mask': uint8 0/1 [512,512]}) out.  warp_temp_folder is accepted and unused (nothing touches the disk).
        With mesher='device' a non-zero mesher status raises RuntimeError (the result is on the host here anyway)."""
        hp, fp = np.asarray(hair_parsing), np.asarray(face_parsing)
        if hp.shape != (IMG, IMG) or fp.shape != (IMG, IMG):
            raise ValueError(f'parsings must be {IMG}x{IMG} label maps, got {hp.shape} and {fp.shape}')
        out = self.warp_batch(hp[None], fp[None], np.asarray(hair_lm_81)[None], np.asarray(face_lm_81)[None],
                              mesher=mesher)[0].cpu().numpy()
        if mesher == 'device' and int(self.last_mesh_status[0]) != 0:
            raise RuntimeError(f'device meshing failed with status {int(self.last_mesh_status[0])} (ch_delaunay_batch)')
        return out.astype('int'), {'hair_mask': (out == HAIR_IDX).astype('uint8')}
