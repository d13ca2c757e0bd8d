"""JPEG files to pixels that are wanted on the device: ch_jpeg_decode_rst (include/ctrlhair_hip.h, csrc/jpeg_decode.hip) Huffman-decodes the
entropy-coded scans of a batch of files there -- in parallel WITHIN each scan, by self-synchronising subsequences (csrc/jpeg_entropy_core.h)
-- and dequantises, inverse-transforms, upsamples and colour-converts them with libjpeg's integer arithmetic; the host reads the markers.

The photos the crop and paste-back jobs read are normally JPEGs, decoded by Pillow on one core in tens of milliseconds each, beside
kernels of a millisecond.  With this module the compressed bytes are uploaded instead (one upload per group of equally shaped files)
and the pixels never exist on the host.  For every stream the device accepts (its status is 0) the pixels are the ones
`Image.open(path).convert('RGB')` (or 'L' for grey files) returns, byte for byte (Pillow on libjpeg-turbo).

Only what the device decodes is parsed: baseline sequential Huffman (SOF0), 8 bits, one scan holding all components, 1 component or 3
(YCbCr; luma sampled 1x1, 2x1 or 2x2, chroma 1x1), 8-bit quantisers, any Huffman tables, with or without a restart interval (DRI and
RST0..RST7, as cameras write them: parse_jpeg_restart; parse_jpeg keeps refusing them).  A file whose restart markers are not where its
interval puts them has status RESTART: libjpeg's resynchronisation of damaged intervals is Pillow's.  Everything else -- and
every stream the device refuses (its status is non-zero) -- goes to Pillow, file by file (dataset.read_rgb / read_gray), so results and
errors are the host path's by construction; JpegDecoder.fallbacks counts those files.  EXIF orientation is not applied (nor by read_rgb).
"""
import re
import struct
from typing import List, Sequence, Tuple

import numpy as np

from .devop import DeviceOp
from .jpegenc import ZIGZAG
from .pngdec import DECODE_MODES, check_decode_mode  # noqa: F401  (one option, one set of names)

TABLE_BYTES = 2048                        # the per-image table block of ch_jpeg_decode (csrc/jpeg_entropy_core.h)
_TABLE_HUFF, _TABLE_HUFF_STRIDE = 192, 272
SAMPLINGS = {0x11: 0, 0x21: 1, 0x22: 2}   # luma sampling byte of SOF0 -> Pillow's subsampling number (4:4:4, 4:2:2, 4:2:0)
MAX_STREAM = 1 << 28
_ALIGN = 16
_MARKER = re.compile(rb'\xff[^\x00]')
_MARKER_NOT_RST = re.compile(rb'\xff[^\x00\xd0-\xd7]')
_SOF_NAMES = {0xC1: 'extended sequential', 0xC2: 'progressive', 0xC3: 'lossless', 0xC5: 'differential sequential', 0xC6: 'differential progressive',
              0xC7: 'differential lossless', 0xC9: 'arithmetic coding', 0xCA: 'arithmetic coding', 0xCB: 'arithmetic coding',
              0xCD: 'arithmetic coding', 0xCE: 'arithmetic coding', 0xCF: 'arithmetic coding'}

STATUS_NAMES = ('OK', 'BAD_CODE', 'BAD_INDEX', 'INPUT_END', 'BLOCKS', 'NOT_SYNCED', 'TOO_LONG', 'MARKER', 'RANGE', 'RESTART')
NOT_SYNCED = 5


class Unsupported(ValueError):
    """parse_jpeg: not a JPEG file of the kind ch_jpeg_decode reads (the reason is the message)."""


def blocks_of(H: int, W: int, C: int, sampling: int) -> int:
    """8x8 blocks of the scan, the dummy blocks of partial MCUs included."""
    hs, vs = ((1, 1), (2, 1), (2, 2))[sampling] if C == 3 else (1, 1)
    return -(-W // (8 * hs)) * -(-H // (8 * vs)) * (hs * vs + 2 if C == 3 else 1)


def stream_bound(H: int, W: int, C: int, sampling: int) -> int:
    """No valid scan is longer: 64 symbols of at most 31 bits per block, every byte stuffed (the header's ch_jpeg_decode)."""
    return min(512 * blocks_of(H, W, C, sampling), MAX_STREAM - 1)


def _check_huffman(cls: int, bits: bytes, vals: bytes) -> None:
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            raise Unsupported('a Huffman table whose lengths are no prefix code')
        code <<= 1
    if cls == 0 and any(v > 15 for v in vals):
        raise Unsupported('a DC Huffman table with a symbol above 15')


def parse_jpeg(data: bytes) -> Tuple[int, int, int, int, bytes, bytes]:
    """A JPEG file -> (H, W, C, sampling, table block, the entropy-coded scan).  sampling: 0 = 4:4:4 (and grey), 1 = 4:2:2, 2 = 4:2:0.
    table block: TABLE_BYTES bytes -- per component its quantiser in natural order, its DC and its AC Huffman table as BITS and HUFFVAL.
    Raises Unsupported for everything outside the module's scope -- a restart interval included: parse_jpeg_restart -- and for a damaged
    container."""
    return _parse(data, False)[:6]


def parse_jpeg_restart(data: bytes) -> Tuple[int, int, int, int, bytes, bytes, int]:
    """parse_jpeg with restart intervals in scope -> (H, W, C, sampling, table block, scan, Ri).  Ri: the DRI segment's MCUs per interval
    (the last one before the scan; 0 without one, and then everything is parse_jpeg's).  With Ri > 0 the scan -- the bytes between the SOS
    header and EOI -- keeps its RST0..RST7 markers; any other marker inside it stays Unsupported."""
    return _parse(data, True)


def _parse(data: bytes, restart_ok: bool):
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        raise Unsupported('no SOI marker')
    pos, quant, huff, frame, jfif, adobe, ri = 2, {}, {}, None, False, None, 0
    while True:
        if pos + 2 > len(data):
            raise Unsupported('truncated: no SOS marker')
        if data[pos] != 0xFF:
            raise Unsupported('bytes between segments')
        m = data[pos + 1]
        if m == 0xFF:                                                          # fill byte
            pos += 1
            continue
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            raise Unsupported(f'marker FF{m:02X} between segments')
        if m == 0xD9:
            raise Unsupported('EOI before any scan')
        if pos + 4 > len(data):
            raise Unsupported('truncated inside a segment')
        n = struct.unpack('>H', data[pos + 2:pos + 4])[0]
        if n < 2 or pos + 2 + n > len(data):
            raise Unsupported('truncated inside a segment')
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m in _SOF_NAMES:
            raise Unsupported(f'{_SOF_NAMES[m]} frame (SOF{m - 0xC0})')
        if m == 0xC0:
            if frame is not None or len(body) < 6:
                raise Unsupported('bad or repeated SOF0')
            P, H, W, C = struct.unpack('>BHHB', body[:6])
            if len(body) != 6 + 3 * C:
                raise Unsupported('bad SOF0')
            frame = (P, H, W, [tuple(body[6 + 3 * k:9 + 3 * k]) for k in range(C)])
        elif m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise Unsupported('16-bit quantiser table')
                if len(body) < 65 or (body[0] & 15) > 3:
                    raise Unsupported('bad DQT')
                quant[body[0] & 15] = body[1:65]
                body = body[65:]
        elif m == 0xC4:
            while body:
                if len(body) < 17 or (body[0] >> 4) > 1 or (body[0] & 15) > 3:
                    raise Unsupported('bad DHT')
                bits = body[1:17]
                k = sum(bits)
                if k > 256 or len(body) < 17 + k:
                    raise Unsupported('bad DHT')
                _check_huffman(body[0] >> 4, bits, body[17:17 + k])
                huff[body[0]] = bits + body[17:17 + k] + bytes(256 - k)
                body = body[17 + k:]
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported('bad DRI')
            if body != b'\0\0' and not restart_ok:
                raise Unsupported('restart interval (DRI)')
            ri = struct.unpack('>H', body)[0]
        elif m == 0xE0 and body[:5] == b'JFIF\0':
            jfif = True
        elif m == 0xEE and body[:5] == b'Adobe' and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            break
    if frame is None:
        raise Unsupported('SOS before SOF0')
    P, H, W, comps = frame
    C = len(comps)
    if P != 8:
        raise Unsupported(f'{P}-bit samples')
    if C not in (1, 3):
        raise Unsupported(f'{C} components')
    if not (1 <= H <= 32768 and 1 <= W <= 32768 and H * W <= 1 << 30):
        raise Unsupported(f'{W}x{H}: sides must be 1..32768 and H * W <= 2^30')
    if C == 3:
        if adobe is not None and adobe != 1:
            raise Unsupported(f'Adobe marker with transform {adobe}')
        if not jfif and adobe is None and bytes(c[0] for c in comps) == b'RGB':
            raise Unsupported('three components that are RGB, not YCbCr')
        if comps[0][1] not in SAMPLINGS or comps[1][1] != 0x11 or comps[2][1] != 0x11:
            raise Unsupported('sampling factors other than 4:4:4, 4:2:2 and 4:2:0')
        sampling = SAMPLINGS[comps[0][1]]
    else:
        if not (1 <= comps[0][1] >> 4 <= 4 and 1 <= comps[0][1] & 15 <= 4):
            raise Unsupported('bad sampling factor')
        sampling = 0
    if len(body) != 4 + 2 * C or body[0] != C:
        raise Unsupported('several scans: the first does not hold all components')
    if [body[1 + 2 * k] for k in range(C)] != [c[0] for c in comps]:
        raise Unsupported('scan components not in frame order')
    if body[1 + 2 * C:] != b'\x00\x3f\x00':
        raise Unsupported('spectral selection or successive approximation in a baseline scan')
    tables = bytearray(TABLE_BYTES)
    for k, (_, _, tq) in enumerate(comps):
        if tq not in quant:
            raise Unsupported(f'quantiser table {tq} is missing')
        q = bytearray(64)
        for z in range(64):
            q[ZIGZAG[z]] = quant[tq][z]
        tables[64 * k:64 * k + 64] = q
        sel = body[2 + 2 * k]
        for cls, ident in ((0, sel >> 4), (1, 0x10 | (sel & 15))):
            if ident not in huff:
                raise Unsupported(f'Huffman table {ident:02x} is missing')
            at = _TABLE_HUFF + (2 * k + cls) * _TABLE_HUFF_STRIDE
            tables[at:at + _TABLE_HUFF_STRIDE] = huff[ident]
    found = (_MARKER_NOT_RST if ri else _MARKER).search(data, pos)
    if found is None:
        raise Unsupported('no EOI marker')
    if data[found.start() + 1] != 0xD9:
        raise Unsupported(f'marker FF{data[found.start() + 1]:02X} inside the scan (a restart marker or a second scan)')
    scan = data[pos:found.start()]
    if len(scan) > stream_bound(H, W, C, sampling):
        raise Unsupported('a scan longer than any valid one')
    return H, W, C, sampling, bytes(tables), scan, ri


class JpegDecoder(DeviceOp):
    """ch_jpeg_decode on one ch_handle.  The constructor needs the library and a GPU; the Pillow fallback is per FILE (see the module)."""

    def __init__(self, handle, device):
        super().__init__(handle, device)
        self.fallbacks = 0

    def upload(self, streams: Sequence[bytes], tables: Sequence[bytes], restart: Sequence[int] = None):
        """N scans and their table blocks -> (device buffer, where the tables and the streams start in it, N[, where the restart intervals
        start]): one buffer -- the offsets table, (restart: the intervals as uint32,) the table blocks, the streams without gaps (each part
        from a multiple of 16 bytes) -- packed in pinned memory and uploaded in one copy.  restart: per stream its Ri (parse_jpeg_restart);
        None: all 0, the buffer and the call of a decoder without restart intervals."""
        N = len(streams)
        if len(tables) != N or any(len(t) != TABLE_BYTES for t in tables):
            raise ValueError(f'JpegDecoder: one table block of {TABLE_BYTES} bytes per stream')
        if restart is not None and (len(restart) != N or any(not 0 <= int(r) <= 0xFFFFFFFF for r in restart)):
            raise ValueError('JpegDecoder: one restart interval (0..2^32 - 1 MCUs) per stream')
        offs = np.zeros(N + 1, np.int64)
        np.cumsum([len(z) for z in streams], out=offs[1:])
        tables_at = 8 * (N + 1) + (-8 * (N + 1)) % _ALIGN
        restart_at = tables_at
        if restart is not None:
            tables_at += 4 * N + (-4 * N) % _ALIGN
        data_at = tables_at + N * TABLE_BYTES
        total = data_at + max(int(offs[N]), 1)
        stage = self._buffer('_pinned', total, pinned=True)
        host = stage[:total].numpy()
        host[:8 * (N + 1)] = np.frombuffer(offs.tobytes(), np.uint8)
        if restart is not None:
            host[restart_at:restart_at + 4 * N] = np.frombuffer(np.asarray([int(r) for r in restart], np.uint32).tobytes(), np.uint8)
        host[tables_at:data_at] = np.frombuffer(b''.join(tables), np.uint8)
        host[data_at:data_at + int(offs[N])] = np.frombuffer(b''.join(streams), np.uint8)
        dev = self._buffer('_in', total)
        dev[:total].copy_(stage[:total], non_blocking=True)
        return (dev, tables_at, data_at, N) if restart is None else (dev, tables_at, data_at, N, restart_at)

    def _reject(self, N, H, W, C, sampling):
        return ValueError(f'JpegDecoder: ch_jpeg_decode rejects N={N}, H={H}, W={W}, C={C}, sampling={sampling} (C 1/3, sampling 0/1/2 and 0 '
                          f'for C = 1, sides 1..32768, H * W <= 2^30, N 1..65535)')

    def launch(self, uploaded, H: int, W: int, C: int, sampling: int, rounds: int = 0):
        """One ch_jpeg_decode call (ch_jpeg_decode_rst when upload() was given restart intervals) on what upload() returned -> (uint8
        [N,H,W,C], int32 [N] statuses), device tensors; no synchronisation."""
        import torch
        dev, tables_at, data_at, N = uploaded[:4]
        need = int(self.handle.lib.ch_jpeg_decode_workspace_bytes(N, H, W, C, sampling))
        if need == 0:
            raise self._reject(N, H, W, C, sampling)
        ws = self._buffer('_ws', need)
        img = torch.empty((N, H, W, C), dtype=torch.uint8, device=self.device)
        status = torch.empty(N, dtype=torch.int32, device=self.device)
        if len(uploaded) == 4:
            self.handle.call('ch_jpeg_decode', dev.data_ptr() + data_at, dev.data_ptr(), dev.data_ptr() + tables_at, N, H, W, C, sampling, rounds,
                             img.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        else:
            self.handle.call('ch_jpeg_decode_rst', dev.data_ptr() + data_at, dev.data_ptr(), dev.data_ptr() + tables_at,
                             dev.data_ptr() + uploaded[4], N, H, W, C, sampling, rounds, img.data_ptr(), status.data_ptr(), ws.data_ptr(),
                             ws.numel(), self._stream())
        return img, status

    def decode_streams(self, streams: Sequence[bytes], tables: Sequence[bytes], H: int, W: int, C: int, sampling: int, rounds: int = 0,
                       restart: Sequence[int] = None):
        """N scans of images of one shape -> (uint8 device tensor [N,H,W,C], int32 device tensor [N] of CH_JPEG_DEC_* statuses).  One
        upload, one ch_jpeg_decode call, one synchronisation at the end (the pinned stage and the input buffer are reused by the next
        call).  rounds: launches of the hand-over between chunks, 0 for the library's default.  restart: per stream its restart interval
        in MCUs, the scans then with their RSTm markers (ch_jpeg_decode_rst); None: none has one."""
        import torch
        if int(self.handle.lib.ch_jpeg_decode_workspace_bytes(len(streams), H, W, C, sampling)) == 0:
            raise self._reject(len(streams), H, W, C, sampling)
        out = self.launch(self.upload(streams, tables, restart), H, W, C, sampling, rounds)
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def decode(self, blobs: Sequence[bytes], rounds: int = 0):
        """JPEG files (bytes) -> (tensors, statuses): per file a uint8 device tensor [H,W,3] ([H,W] for grey files) and the CH_JPEG_DEC_*
        status of its scan (non-zero: the pixels are unspecified).  Files are grouped by (H, W, C, sampling), one ch_jpeg_decode call per
        group, whatever the files' restart intervals.  Raises Unsupported for a file parse_jpeg_restart refuses."""
        parsed = [parse_jpeg_restart(b) for b in blobs]
        groups = {}
        for i, p in enumerate(parsed):
            groups.setdefault(p[:4], []).append(i)
        tensors, statuses = [None] * len(parsed), [0] * len(parsed)
        for (H, W, C, sampling), idx in groups.items():
            restart = [parsed[i][6] for i in idx]
            img, status = self.decode_streams([parsed[i][5] for i in idx], [parsed[i][4] for i in idx], H, W, C, sampling, rounds,
                                              restart if any(restart) else None)
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
            if p.lower().endswith(('.jpg', '.jpeg')):
                with open(p, 'rb') as f:
                    data = f.read()
                try:
                    C = parse_jpeg_restart(data)[2]
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
                    if not gray and t.dim() == 2:
                        t = t[:, :, None].expand(-1, -1, 3)
                    out[i] = t.contiguous()
        for i, p in enumerate(paths):
            if out[i] is None:
                self.fallbacks += 1
                out[i] = torch.from_numpy(np.array(host_read(p))).to(self.device)
        return out

    def read_rgb(self, paths: Sequence[str]) -> List:
        """dataset.read_rgb of every path, as uint8 device tensors [H,W,3]: grey files are replicated, as convert('RGB') does."""
        return self._read(paths, gray=False)

    def read_gray(self, paths: Sequence[str]) -> List:
        """dataset.read_gray of every path, as uint8 device tensors [H,W]; only grey files are decoded on the device."""
        return self._read(paths, gray=True)
