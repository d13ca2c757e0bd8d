"""PNG files to pixels that are wanted on the device: ch_png_decode (include/ctrlhair_hip.h, csrc/png_decode.hip) inflates the zlib
streams of a batch of files there, one wavefront per file, and undoes the row filters; the host reads the container.

The dataset jobs read the crops and label maps the project's own jobs wrote, decode them with Pillow on one core, upload the pixels and
run a sub-millisecond kernel.  With this module the compressed bytes are uploaded instead (one upload per group of equally sized files)
and the pixels never exist on the host.  What is left for the host is the container: signature, chunk walk, CRC-32 (zlib.crc32, over the
chunk types and the COMPRESSED bytes), the IDAT payloads concatenated.

Only what the device decodes is parsed: bit depth 8, colour type 0 / 2 / 6 (grey, RGB, RGBA), not interlaced.  Everything else -- and
every stream the device refuses (its status is non-zero) -- goes to Pillow, file by file (dataset.read_rgb / read_gray), so results and
errors are the host path's by construction; PngDecoder.fallbacks counts those files.
"""
import struct
import zlib
from typing import List, Sequence, Tuple

import numpy as np

from .devop import DeviceOp
from .pngenc import PNG_SIGNATURE

CHANNELS = {0: 1, 2: 3, 6: 4}             # PNG colour type -> channels, bit depth 8
DECODE_MODES = ('host', 'device')
_ALIGN = 16                               # the first stream of an upload starts on a multiple of this


class Unsupported(ValueError):
    """parse_png: not a PNG file of the kind ch_png_decode reads (the reason is the message)."""


def check_decode_mode(decode: str) -> str:
    if decode not in DECODE_MODES:
        raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
    return decode


def parse_png(data: bytes) -> Tuple[int, int, int, bytes]:
    """A PNG file -> (H, W, C, the zlib stream of its filtered rows).  Every chunk's CRC is checked; ancillary chunks are skipped (Pillow's
    convert('RGB') / convert('L') applies neither gAMA nor tRNS).  Raises Unsupported for anything but 8-bit grey / RGB / RGBA without
    interlace, for a damaged container and for a CRC mismatch."""
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise Unsupported('no PNG signature')
    pos, header, idat, ended = 8, None, [], False
    while not ended:
        if pos + 8 > len(data):
            raise Unsupported('truncated: no IEND chunk')
        length, kind = struct.unpack('>I4s', data[pos:pos + 8])
        if pos + 12 + length > len(data):
            raise Unsupported(f'truncated inside a {kind!r} chunk')
        body = data[pos + 8:pos + 8 + length]
        if struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(body, zlib.crc32(kind)) & 0xFFFFFFFF):
            raise Unsupported(f'CRC mismatch in a {kind!r} chunk')
        pos += 12 + length
        if header is None and kind != b'IHDR':
            raise Unsupported('the first chunk is not IHDR')
        if kind == b'IHDR':
            if header is not None or length != 13:
                raise Unsupported('bad IHDR')
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            ended = True
        elif not kind[0] & 0x20 and kind != b'PLTE':
            raise Unsupported(f'unknown critical chunk {kind!r}')
    W, H, depth, colour, compression, filter_method, interlace = header
    if depth != 8:
        raise Unsupported(f'bit depth {depth}')
    if colour not in CHANNELS:
        raise Unsupported(f'colour type {colour} (palette or grey with alpha)')
    if compression != 0 or filter_method != 0:
        raise Unsupported('unknown compression or filter method')
    if interlace != 0:
        raise Unsupported('interlaced (Adam7)')
    if not (1 <= H <= 32768 and 1 <= W <= 32768 and H * W <= 1 << 30):
        raise Unsupported(f'{W}x{H}: sides must be 1..32768 and H * W <= 2^30')
    if not idat:
        raise Unsupported('no IDAT chunk')
    return H, W, CHANNELS[colour], b''.join(idat)


class PngDecoder(DeviceOp):
    """ch_png_decode on one ch_handle.  The constructor needs the library and a GPU; the Pillow fallback is per FILE (see the module)."""

    def __init__(self, handle, device):
        super().__init__(handle, device)
        self.fallbacks = 0

    def upload(self, streams: Sequence[bytes]):
        """N zlib streams -> (device buffer, where the streams start in it, N): one buffer -- the offsets table, then (from a multiple of
        16 bytes) the streams without gaps, offsets counting from the first stream -- packed in pinned memory and uploaded in one copy."""
        N = len(streams)
        offs = np.zeros(N + 1, np.int64)
        np.cumsum([len(z) for z in streams], out=offs[1:])
        data_at = 8 * (N + 1) + (-8 * (N + 1)) % _ALIGN
        total = data_at + max(int(offs[N]), 1)
        stage = self._buffer('_pinned', total, pinned=True)
        host = stage[:total].numpy()
        host[:8 * (N + 1)] = np.frombuffer(offs.tobytes(), np.uint8)
        host[data_at:data_at + int(offs[N])] = np.frombuffer(b''.join(streams), np.uint8)
        dev = self._buffer('_in', total)
        dev[:total].copy_(stage[:total], non_blocking=True)
        return dev, data_at, N

    def launch(self, uploaded, H: int, W: int, C: int):
        """One ch_png_decode call on what upload() returned -> (uint8 [N,H,W,C], int32 [N] statuses), device tensors; no synchronisation."""
        import torch
        dev, data_at, N = uploaded
        need = int(self.handle.lib.ch_png_decode_workspace_bytes(N, H, W, C))
        if need == 0:
            raise ValueError(f'PngDecoder: ch_png_decode rejects N={N}, H={H}, W={W}, C={C} (C 1/3/4, sides 1..32768, H * W <= 2^30, N 1..65535)')
        ws = self._buffer('_ws', need)
        img = torch.empty((N, H, W, C), dtype=torch.uint8, device=self.device)
        status = torch.empty(N, dtype=torch.int32, device=self.device)
        self.handle.call('ch_png_decode', dev.data_ptr() + data_at, dev.data_ptr(), N, H, W, C, img.data_ptr(), status.data_ptr(), ws.data_ptr(),
                         ws.numel(), self._stream())
        return img, status

    def decode_streams(self, streams: Sequence[bytes], H: int, W: int, C: int):
        """N zlib streams of images of one size -> (uint8 device tensor [N,H,W,C], int32 device tensor [N] of CH_PNG_DEC_* statuses).
        One upload, one ch_png_decode call, one synchronisation at the end (the pinned stage and the input buffer are reused by the
        next call)."""
        import torch
        if int(self.handle.lib.ch_png_decode_workspace_bytes(len(streams), H, W, C)) == 0:
            raise ValueError(f'PngDecoder: ch_png_decode rejects N={len(streams)}, H={H}, W={W}, C={C} (C 1/3/4, sides 1..32768, '
                             f'H * W <= 2^30, N 1..65535)')
        out = self.launch(self.upload(streams), H, W, C)
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def decode(self, blobs: Sequence[bytes]):
        """PNG files (bytes) -> (tensors, statuses): per file a uint8 device tensor [H,W,C] ([H,W] for C = 1) and the CH_PNG_DEC_* status
        of its stream (non-zero: the pixels are unspecified).  Files are grouped by (H, W, C), one ch_png_decode call per group.
        Raises Unsupported for a file parse_png refuses."""
        parsed = [parse_png(b) for b in blobs]
        groups = {}
        for i, (H, W, C, _) in enumerate(parsed):
            groups.setdefault((H, W, C), []).append(i)
        tensors, statuses = [None] * len(parsed), [0] * len(parsed)
        for (H, W, C), idx in groups.items():
            img, status = self.decode_streams([parsed[i][3] for i in idx], H, W, C)
            status = status.cpu().tolist()
            for k, i in enumerate(idx):
                tensors[i] = img[k, :, :, 0] if C == 1 else img[k]
                statuses[i] = int(status[k])
        return tensors, statuses

    def _read(self, paths: Sequence[str], gray: bool) -> List:
        import torch
        from . import dataset
        host_read = dataset.read_gray if gray else dataset.read_rgb
        paths = list(paths)
        out, blobs, where = [None] * len(paths), [], []
        for i, p in enumerate(paths):
            if p.lower().endswith('.png'):
                with open(p, 'rb') as f:
                    data = f.read()
                try:
                    C = parse_png(data)[2]
                except Unsupported:
                    continue
                if gray and C != 1:                                             # convert('L') weighs the channels: Pillow's arithmetic
                    continue
                blobs.append(data)
                where.append(i)
        if blobs:
            tensors, statuses = self.decode(blobs)
            for i, t, s in zip(where, tensors, statuses):
                if s == 0:
                    if not gray:
                        t = t[:, :, None].expand(-1, -1, 3) if t.dim() == 2 else t[:, :, :3]
                    out[i] = t.contiguous()
        for i, p in enumerate(paths):
            if out[i] is None:
                self.fallbacks += 1
                out[i] = torch.from_numpy(np.array(host_read(p))).to(self.device)
        return out

    def read_rgb(self, paths: Sequence[str]) -> List:
        """dataset.read_rgb of every path, as uint8 device tensors [H,W,3]: RGBA drops alpha, grey is replicated."""
        return self._read(paths, gray=False)

    def read_gray(self, paths: Sequence[str]) -> List:
        """dataset.read_gray of every path, as uint8 device tensors [H,W]; only grey files are decoded on the device."""
        return self._read(paths, gray=True)
