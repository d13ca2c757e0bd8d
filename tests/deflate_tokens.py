"""A small pure-Python inflate (RFC 1951: stored, fixed and dynamic blocks) that keeps what zlib throws away: the token list --
('L', byte) and ('M', length, distance) -- and the block boundaries.  Test code only; slow, meant for streams of some ten thousand bytes."""
import collections
import zlib

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

# btype 0 stored / 1 fixed / 2 dynamic; tokens[tok_start:tok_end] are the block's (none for a stored block), out[out_start:out_end] its
# bytes, [bit_start, bit_end) its bits in the raw deflate data; dist_lengths: the distance code lengths of a dynamic block, else None
Block = collections.namedtuple('Block', 'btype final tok_start tok_end out_start out_end bit_start bit_end dist_lengths')


class _Bits:
    def __init__(self, data: bytes):
        self.data, self.pos = data, 0

    def peek(self, n: int) -> int:                                                         # n <= 16 bits, least significant first; zeros past the end
        b = self.pos >> 3
        return (int.from_bytes(self.data[b:b + 3], 'little') >> (self.pos & 7)) & ((1 << n) - 1)

    def skip(self, n: int) -> None:
        self.pos += n
        if self.pos > 8 * len(self.data):
            raise ValueError('deflate data ends inside a block')

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.skip(n)
        return v


def _table(lengths):
    """Canonical Huffman code (RFC 1951 3.2.2): {(length, code): symbol}."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def _symbol(br: _Bits, table) -> int:
    w, code = br.peek(15), 0
    for l in range(1, 16):
        code = (code << 1) | (w & 1)                                                       # Huffman codes come most significant bit first
        w >>= 1
        if (l, code) in table:
            br.skip(l)
            return table[(l, code)]
    raise ValueError('no such Huffman code')


FIXED_LL = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = _table([5] * 30)


def inflate(raw: bytes):
    """Raw deflate data -> (tokens, decoded bytes, blocks, bytes consumed)."""
    br = _Bits(bytes(raw))
    tokens, out, blocks = [], bytearray(), []
    final = 0
    while not final:
        bit_start, tok_start, out_start = br.pos, len(tokens), len(out)
        final, btype = br.take(1), br.take(2)
        dist_lengths = None
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.take(16), br.take(16)
            if n != (~nn & 0xFFFF):
                raise ValueError('stored block: LEN and NLEN disagree')
            a = br.pos >> 3
            if a + n > len(br.data):
                raise ValueError('stored block runs past the data')
            out += br.data[a:a + n]
            br.pos += 8 * n
        elif btype in (1, 2):
            if btype == 1:
                ll, dt = FIXED_LL, FIXED_DIST
            else:
                hlit, hdist, hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = br.take(3)
                clt = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(br, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ValueError('repeat code with nothing before it')
                        lens += [lens[-1]] * (3 + br.take(2))
                    elif s == 17:
                        lens += [0] * (3 + br.take(3))
                    else:
                        lens += [0] * (11 + br.take(7))
                if len(lens) != hlit + hdist:
                    raise ValueError('code lengths overrun the header counts')
                dist_lengths = lens[hlit:]
                ll, dt = _table(lens[:hlit]), _table(dist_lengths)
            while True:
                s = _symbol(br, ll)
                if s < 256:
                    tokens.append(('L', s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError('length symbol beyond 285')
                    length = LENGTH_BASE[s - 257] + br.take(LENGTH_EXTRA[s - 257])
                    ds = _symbol(br, dt)
                    if ds > 29:
                        raise ValueError('distance symbol beyond 29')
                    dist = DIST_BASE[ds] + br.take(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise ValueError('match reaches before the start of the data')
                    tokens.append(('M', length, dist))
                    for _ in range(length):
                        out.append(out[-dist])
        else:
            raise ValueError('block type 3')
        blocks.append(Block(btype, final, tok_start, len(tokens), out_start, len(out), bit_start, br.pos, dist_lengths))
    return tokens, bytes(out), blocks, (br.pos + 7) >> 3


def inflate_zlib(stream: bytes):
    """A zlib stream (RFC 1950) -> (tokens, decoded bytes, blocks); header, Adler-32 and the absence of trailing bytes are checked."""
    stream = bytes(stream)
    if len(stream) < 6 or (stream[0] & 15) != 8 or ((stream[0] << 8) | stream[1]) % 31 or stream[1] & 32:
        raise ValueError('not a zlib stream without a preset dictionary')
    tokens, out, blocks, used = inflate(stream[2:])
    tail = stream[2 + used:]
    if len(tail) != 4 or int.from_bytes(tail, 'big') != (zlib.adler32(out) & 0xFFFFFFFF):
        raise ValueError('Adler-32 missing, wrong, or followed by more bytes')
    return tokens, out, blocks
