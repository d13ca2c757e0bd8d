"""JPEG files from pixels that are already on the device: ch_jpeg_encode (include/ctrlhair_hip.h, csrc/jpeg_encode.hip) converts the
colours, transforms, quantises and Huffman-codes them there and hands back one entropy-coded scan per image; the host adds the markers.

The photos the crop and paste-back jobs work on are normally JPEGs, and both jobs keep the input's file name.  Downloading a
photo-sized result and giving it to Pillow (one core) costs far more than the kernels that made it.  With this module only the
compressed bytes cross the bus: one download of the N scan lengths, then one download of exactly those bytes.  What is left for the host
is the container: SOI, APP0, the quantisation tables, SOF0, the Huffman tables, SOS, the scan, EOI.

Unlike the PNG encoder's, these files are not merely equivalent: the device restates libjpeg's integer arithmetic, and wrap_jpeg writes
Pillow's markers in Pillow's order, so a file equals what `Image.save(path, quality=q, subsampling=s)` writes for the same pixels, byte
for byte (libjpeg / libjpeg-turbo, optimize=False, no EXIF / ICC).  `Image.save(path)` without options is quality 75, 4:2:0 for RGB.
Baseline only: no progressive mode, no optimised Huffman tables, no restart markers, no 4:2:2.
"""
import struct
from typing import List, Sequence

import numpy as np

from .devop import DeviceOp
from .photometa import EXIF_MAX, per_image      # (shared with pngenc and the jobs; re-exported here)

JPEG_MODES = ('host', 'device')
SUBSAMPLINGS = (0, 2)                     # Pillow's numbering: 0 = 4:4:4, 2 = 4:2:0
SUBSAMPLING_NAMES = {'444': 0, '420': 2}  # the command line's names

# ITU-T T.81 Annex K.1, natural (row-major) order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    return tuple(order)


ZIGZAG = _zigzag()                        # natural index of zigzag position k

# Annex K.3: (number of codes of each length 1..16, the symbols in code order).  The AC symbols are run << 4 | size.
DHT_DC_LUMA = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12)))
DHT_DC_CHROMA = (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12)))
DHT_AC_LUMA = (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]), bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
    'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'))
DHT_AC_CHROMA = (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849'
    '4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5'
    'c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))


def check_jpeg_mode(jpeg: str) -> str:
    if jpeg not in JPEG_MODES:
        raise ValueError(f"jpeg must be 'host' or 'device', got {jpeg!r}")
    return jpeg


def check_jpeg_params(quality, subsampling) -> tuple:
    """(quality, subsampling) as ints, checked as the library checks them: quality 1..100; subsampling 0 (4:4:4) or 2 (4:2:0), or the
    command line's '444' / '420'."""
    if isinstance(subsampling, str):
        if subsampling not in SUBSAMPLING_NAMES:
            raise ValueError(f"jpeg subsampling must be 0 / '444' or 2 / '420', got {subsampling!r}")
        subsampling = SUBSAMPLING_NAMES[subsampling]
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f'jpeg quality must be an int in 1..100, got {quality!r}')
    if isinstance(subsampling, bool) or not isinstance(subsampling, (int, np.integer)) or int(subsampling) not in SUBSAMPLINGS:
        raise ValueError(f"jpeg subsampling must be 0 / '444' or 2 / '420', got {subsampling!r}")
    return int(quality), int(subsampling)


def quant_tables(quality: int):
    """(luma, chroma): uint8 [64] each in natural order -- libjpeg's jpeg_quality_scaling and its baseline clamp."""
    q, _ = check_jpeg_params(quality, 0)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], np.uint8) for base in (BASE_LUMA, BASE_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


ICC_CHUNK = 65519                         # profile bytes per APP2 segment: 65533 - len('ICC_PROFILE\0', index, count)


def metadata_segments(exif: bytes = None, icc_profile: bytes = None) -> bytes:
    """The segments Pillow's save(exif=, icc_profile=) puts between APP0 and the first DQT: APP1 with the EXIF block as given (it starts
    with 'Exif\\0\\0'), then the profile cut into APP2 'ICC_PROFILE\\0' segments of at most 65519 profile bytes, numbered from 1."""
    out = []
    if exif:
        if len(exif) > EXIF_MAX:
            raise ValueError('EXIF data is too long')             # Pillow's own refusal, in its words
        out.append(_segment(0xE1, bytes(exif)))
    if icc_profile:
        chunks = [bytes(icc_profile[a:a + ICC_CHUNK]) for a in range(0, len(icc_profile), ICC_CHUNK)]
        if len(chunks) > 255:
            raise ValueError(f'ICC profile of {len(icc_profile)} bytes needs more than 255 APP2 segments')
        out += [_segment(0xE2, b'ICC_PROFILE\x00' + bytes([i + 1, len(chunks)]) + c) for i, c in enumerate(chunks)]
    return b''.join(out)


def wrap_jpeg(scan: bytes, H: int, W: int, C: int, quality: int = 75, subsampling: int = 2, exif: bytes = None,
              icc_profile: bytes = None) -> bytes:
    """A JPEG file around the entropy-coded scan, marker for marker what Pillow writes: SOI, APP0 (JFIF 1.01, no units, density 1 x 1),
    with exif / icc_profile the segments of metadata_segments, one DQT per table in zigzag order, SOF0, one DHT per table, SOS, the
    scan, EOI.  C = 1: one table of each kind.  The luma sampling factor is 2 x 2 for subsampling 2 and 1 x 1 for 0 -- for grey as
    well, where it changes nothing but that byte."""
    if C not in (1, 3):
        raise ValueError(f'wrap_jpeg: C must be 1 or 3, got {C}')
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError('wrap_jpeg: H and W must be in 1..65535')
    quality, subsampling = check_jpeg_params(quality, subsampling)
    parts = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'), metadata_segments(exif, icc_profile)]
    for k, q in enumerate(quant_tables(quality)[:1 if C == 1 else 2]):
        parts.append(_segment(0xDB, bytes([k]) + bytes(int(q[i]) for i in ZIGZAG)))
    comps = [(1, 0x22 if subsampling == 2 else 0x11, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if C == 3 else [])
    parts.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, C) + b''.join(bytes(c) for c in comps)))
    tables = [(0x00, DHT_DC_LUMA), (0x10, DHT_AC_LUMA)] + ([(0x01, DHT_DC_CHROMA), (0x11, DHT_AC_CHROMA)] if C == 3 else [])
    for ident, (bits, vals) in tables:
        parts.append(_segment(0xC4, bytes([ident]) + bits + vals))
    selectors = [(1, 0x00)] + ([(2, 0x11), (3, 0x11)] if C == 3 else [])
    parts.append(_segment(0xDA, bytes([C]) + b''.join(bytes(s) for s in selectors) + b'\x00\x3f\x00'))
    parts += [bytes(scan), b'\xff\xd9']
    return b''.join(parts)


class JpegEncoder(DeviceOp):
    """ch_jpeg_encode on one ch_handle.  No CPU fallback: the constructor needs the library and a GPU."""

    @staticmethod
    def _shape(images):
        import torch
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() not in (3, 4):
            raise ValueError('JpegEncoder: images must be a uint8 tensor [N,H,W,C] or [N,H,W]')
        N, H, W = (int(v) for v in images.shape[:3])
        C = int(images.shape[3]) if images.dim() == 4 else 1
        if C not in (1, 3):
            raise ValueError(f'JpegEncoder: C must be 1 (grey) or 3 (RGB), got {C}')
        return N, H, W, C

    def scans(self, images, quality: int = 75, subsampling: int = 2) -> List[bytes]:
        """uint8 device tensor [N,H,W,C] or [N,H,W] -> the N entropy-coded scans (bytes).  Two downloads: the lengths, then the bytes."""
        import torch
        N, H, W, C = self._shape(images)
        quality, subsampling = check_jpeg_params(quality, subsampling)
        x = images.to(self.device).contiguous()
        if N == 0:
            return []
        lib = self.handle.lib
        bound, need = int(lib.ch_jpeg_scan_bound(H, W, C, subsampling)), int(lib.ch_jpeg_encode_workspace_bytes(N, H, W, C, subsampling))
        if bound == 0 or need == 0:
            raise ValueError(f'JpegEncoder: ch_jpeg_encode rejects N={N}, H={H}, W={W} (sides 1..32768, H * W <= 2^30, N <= 65535)')
        ws, out = self._buffer('_ws', need), self._buffer('_out', N * bound)
        sizes = torch.empty(N, dtype=torch.int64, device=self.device)
        self.handle.call('ch_jpeg_encode', x.data_ptr(), N, H, W, C, quality, subsampling, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                         ws.numel(), self._stream())
        return self._fetch_ragged(out, bound, sizes, 1, 'ch_jpeg_encode returned scan lengths')

    def encode(self, images, quality: int = 75, subsampling: int = 2, exif: Sequence = None, icc_profile: Sequence = None) -> List[bytes]:
        """uint8 device tensor [N,H,W,C] or [N,H,W] -> N whole JPEG files (bytes).  exif / icc_profile: per image a bytes object or None
        (lists of N), written as Pillow's save(exif=, icc_profile=) writes them."""
        N, H, W, C = self._shape(images)
        quality, subsampling = check_jpeg_params(quality, subsampling)
        exif, icc_profile = per_image(exif, N, 'exif'), per_image(icc_profile, N, 'icc_profile')
        return [wrap_jpeg(s, H, W, C, quality, subsampling, e, p) for s, e, p in zip(self.scans(images, quality, subsampling), exif, icc_profile)]

    def write(self, paths: Sequence[str], images, quality: int = 75, subsampling: int = 2, exif: Sequence = None,
              icc_profile: Sequence = None) -> None:
        """Encode images [N,...] and write file n to paths[n]."""
        paths = list(paths)
        if len(paths) != int(images.shape[0]):
            raise ValueError(f'JpegEncoder.write: {len(paths)} paths for {int(images.shape[0])} images')
        for path, jpg in zip(paths, self.encode(images, quality, subsampling, exif, icc_profile)):
            with open(path, 'wb') as f:
                f.write(jpg)
