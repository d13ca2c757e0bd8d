"""PNG files from pixels that are already on the device: ch_png_encode (include/ctrlhair_hip.h, csrc/png_encode.hip) filters the rows and
deflates them there, chunk by chunk, and hands back one complete zlib stream per image; the host adds the container.

Every dataset-scale job here ends with uint8 pixels on the device.  Downloading them whole and giving them to Pillow (row filters, then
zlib at level 6 on one core) costs more than the kernels that made them.  With this module only the compressed bytes cross the bus:
one download of the N stream lengths, then one download of exactly those bytes.  What is left for the host is the container --
signature, IHDR, the stream cut into IDAT chunks, IEND -- and PNG's CRC-32, which runs over the chunk types and the COMPRESSED bytes only
(zlib.crc32; the pixels' own checksum, the Adler-32 inside the zlib stream, is computed on the device).

Pixels decode exactly; the file bytes are NOT those of Pillow or of any zlib level (another deflate of the same filtered bytes), and they
depend on ch_png_chunk_bytes().

distances=(...) on streams / encode / write: up to three byte distances at which the image repeats itself -- the column pitch of a
contact sheet (ContactSheet.png_distances), a tile period, a row stride.  ch_png_encode_dist then also codes matches at those distances
(the deflate stage alone sees distance 1 only); the pixels are the same, the file is smaller where the layout repeats.
"""
import ctypes
import struct
import zlib
from typing import List, Sequence

import numpy as np

from .devop import DeviceOp

ADLER_MOD = 65521
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}          # channels -> PNG colour type (grey, RGB, RGBA), bit depth 8
IDAT_MAX = 1 << 20                        # bytes of zlib stream per IDAT chunk (any split is valid; libpng's default writes far smaller ones)
PNG_MODES = ('host', 'device')
MAX_DISTANCES = 3                         # caller-given match distances of ch_png_encode_dist


def check_png_mode(png: str) -> str:
    if png not in PNG_MODES:
        raise ValueError(f"png must be 'host' or 'device', got {png!r}")
    return png


def check_distances(distances: Sequence[int]) -> tuple:
    """The further match distances of ch_png_encode_dist as a tuple of ints, checked as the library checks them: at most three, each in
    2..32767 (distance 1 is always present), pairwise distinct."""
    try:
        dist = tuple(distances)
    except TypeError:
        raise ValueError(f'PngEncoder: distances must be a sequence of at most three ints, got {distances!r}') from None
    if len(dist) > MAX_DISTANCES:
        raise ValueError(f'PngEncoder: at most {MAX_DISTANCES} distances, got {len(dist)}')
    for d in dist:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 2 <= int(d) <= 32767:
            raise ValueError(f'PngEncoder: every distance must be an int in 2..32767 (distance 1 is always present), got {d!r}')
    dist = tuple(int(d) for d in dist)
    if len(set(dist)) != len(dist):
        raise ValueError(f'PngEncoder: distances must be pairwise distinct, got {dist}')
    return dist


def adler32_combine(a1: int, a2: int, len2: int) -> int:
    """Adler-32 of the concatenation X + Y from a1 = adler32(X), a2 = adler32(Y) and len2 = len(Y): what the gather kernel does with
    the per-chunk sums (there all at once: B = F + sum over bytes of (F - position) * byte, every chunk adding its share)."""
    s1, b1 = a1 & 0xFFFF, (a1 >> 16) & 0xFFFF
    s2, b2 = a2 & 0xFFFF, (a2 >> 16) & 0xFFFF
    # Y alone starts from A = 1; behind X it starts from A = s1: every one of its len2 steps adds (s1 - 1) more to B
    a = (s1 + s2 - 1) % ADLER_MOD
    b = (b1 + b2 + (len2 % ADLER_MOD) * (s1 - 1)) % ADLER_MOD
    return (b << 16) | a


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF)


def wrap_png(zlib_stream: bytes, H: int, W: int, C: int, exif: bytes = None, icc_profile: bytes = None) -> bytes:
    """A PNG file around the zlib stream of its filtered rows: 8-bit, colour type 0 / 2 / 6 for C = 1 / 3 / 4, not interlaced.
    icc_profile: an iCCP chunk (profile name 'ICC Profile', as Pillow names it, deflated); exif: an eXIf chunk, whose payload is the
    EXIF block without the 'Exif\\0\\0' prefix JPEG's APP1 carries; both before the first IDAT.  Pillow reads both back as given."""
    if C not in COLOUR_TYPE:
        raise ValueError(f'wrap_png: C must be 1, 3 or 4, got {C}')
    if H < 1 or W < 1:
        raise ValueError('wrap_png: H and W must be positive')
    z = bytes(zlib_stream)
    parts = [PNG_SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, COLOUR_TYPE[C], 0, 0, 0))]
    if icc_profile:
        parts.append(_chunk(b'iCCP', b'ICC Profile\x00\x00' + zlib.compress(bytes(icc_profile))))
    if exif:
        exif = bytes(exif)
        parts.append(_chunk(b'eXIf', exif[6:] if exif.startswith(b'Exif\x00\x00') else exif))
    for a in range(0, max(len(z), 1), IDAT_MAX):
        parts.append(_chunk(b'IDAT', z[a:a + IDAT_MAX]))
    parts.append(_chunk(b'IEND', b''))
    return b''.join(parts)


class PngEncoder(DeviceOp):
    """ch_png_encode / ch_png_encode_dist on one ch_handle.  No CPU fallback: the constructor needs the library and a GPU."""

    def __init__(self, handle, device):
        super().__init__(handle, device)
        self.chunk = int(handle.lib.ch_png_chunk_bytes())

    def streams(self, images, filter: int = -1, distances: Sequence[int] = ()) -> List[bytes]:
        """uint8 device tensor [N,H,W,C] or [N,H,W] -> the N zlib streams (bytes).  Two downloads: the lengths, then the bytes.
        distances: up to three further match distances in bytes of the filtered stream (check_distances; ch_png_encode_dist); empty:
        ch_png_encode, distance-1 runs only."""
        import torch
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() not in (3, 4):
            raise ValueError('PngEncoder: images must be a uint8 tensor [N,H,W,C] or [N,H,W]')
        x = images.to(self.device).contiguous()
        N, H, W = (int(v) for v in x.shape[:3])
        C = int(x.shape[3]) if x.dim() == 4 else 1
        if C not in COLOUR_TYPE:
            raise ValueError(f'PngEncoder: C must be 1, 3 or 4, got {C}')
        if not -1 <= int(filter) <= 4:
            raise ValueError(f'PngEncoder: filter must be -1 (adaptive) or 0..4, got {filter}')
        dist = check_distances(distances)
        if N == 0:
            return []
        lib = self.handle.lib
        bound, need = int(lib.ch_png_zlib_bound(H, W, C)), int(lib.ch_png_encode_workspace_bytes(N, H, W, C))
        if bound == 0 or need == 0:
            raise ValueError(f'PngEncoder: ch_png_encode rejects N={N}, H={H}, W={W} (sides 1..32768, H * W <= 2^30, N <= 65535)')
        ws, out = self._buffer('_ws', need), self._buffer('_out', N * bound)
        sizes = torch.empty(N, dtype=torch.int64, device=self.device)
        if dist:
            self.handle.call('ch_png_encode_dist', x.data_ptr(), N, H, W, C, int(filter), (ctypes.c_int * len(dist))(*dist), len(dist),
                             out.data_ptr(), sizes.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        else:
            self.handle.call('ch_png_encode', x.data_ptr(), N, H, W, C, int(filter), out.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                             ws.numel(), self._stream())
        return self._fetch_ragged(out, bound, sizes, 8, 'ch_png_encode returned stream lengths')

    def encode(self, images, filter: int = -1, distances: Sequence[int] = (), exif: Sequence = None, icc_profile: Sequence = None) -> List[bytes]:
        """uint8 device tensor [N,H,W,C] or [N,H,W] -> N whole PNG files (bytes).  exif / icc_profile: per image a bytes object or None
        (lists of N): the eXIf and iCCP chunks of wrap_png."""
        from .photometa import per_image
        N, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
        C = int(images.shape[3]) if images.dim() == 4 else 1
        exif, icc_profile = per_image(exif, N, 'exif'), per_image(icc_profile, N, 'icc_profile')
        return [wrap_png(z, H, W, C, e, p) for z, e, p in zip(self.streams(images, filter, distances), exif, icc_profile)]

    def write(self, paths: Sequence[str], images, filter: int = -1, distances: Sequence[int] = (), exif: Sequence = None,
              icc_profile: Sequence = None) -> None:
        """Encode images [N,...] and write file n to paths[n]."""
        paths = list(paths)
        if len(paths) != int(images.shape[0]):
            raise ValueError(f'PngEncoder.write: {len(paths)} paths for {int(images.shape[0])} images')
        for path, png in zip(paths, self.encode(images, filter, distances, exif, icc_profile)):
            with open(path, 'wb') as f:
                f.write(png)
