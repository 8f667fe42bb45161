"""
A small deflate writer for the PNG decoder's tests (TEST INFRASTRUCTURE ONLY): streams whose tokens the test chooses, which zlib
never writes on its own - every match length, chosen distances, blocks that end inside a byte, dynamic headers with a chosen
run-length coding.  Tokens are ("lit", byte) and ("match", length, distance).  Blocks: stored, fixed Huffman and dynamic Huffman
from tokens, or whatever zlib makes of some bytes (`zlib_blocks`, at a byte boundary).  `expand` gives the bytes a token list
stands for, `zlib_stream` wraps a deflate body with the zlib header and the Adler-32.
"""
import struct
import zlib

CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def lit(b):
    return ("lit", int(b))


def match(length, distance):
    assert 3 <= length <= 258 and 1 <= distance <= 32768
    return ("match", int(length), int(distance))


def expand(tokens, history=b""):
    out = bytearray(history)
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            _, n, d = t
            assert d <= len(out), "a distance beyond the start"
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(history):])


def length_symbol(n):
    """(symbol, extra bits, extra value) of a match length"""
    if n == 258:
        return 285, 0, 0
    if n < 11:
        return 254 + n, 0, 0
    e = (n - 3).bit_length() - 3
    base_index = ((n - 3) >> e) - 4
    return 265 + 4 * (e - 1) + base_index, e, (n - 3) & ((1 << e) - 1)


def distance_symbol(d):
    if d < 5:
        return d - 1, 0, 0
    e = (d - 1).bit_length() - 2
    return 2 * e + 2 + (((d - 1) >> e) & 1), e, (d - 1) & ((1 << e) - 1)


def canonical_codes(lengths):
    """symbol -> (code, length) of the canonical prefix code with these lengths (0: no code)"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def complete_lengths(symbols, alphabet):
    """lengths of a complete prefix code over `symbols` (at least two), the other symbols of the alphabet unused: with
    m = ceil(log2 k), 2^m - k codes of m - 1 bits (the first symbols) and the rest of m bits"""
    k = len(symbols)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    lengths = [0] * alphabet
    for i, s in enumerate(symbols):
        lengths[s] = m - 1 if i < short else m
    return lengths


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class DeflateWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):  # first bit lowest, as header fields and extra bits go
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):  # a Huffman code: first bit highest
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def aligned(self):
        return self.n == 0

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.bits(int(final), 1)
        self.bits(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen)
        self.out += data

    def _tokens(self, tokens, lit_codes, dist_codes):
        for t in tokens:
            if t[0] == "lit":
                self.code(*lit_codes[t[1]])
            elif t[0] == "sym":  # a raw literal/length symbol, for damaged streams
                self.code(*lit_codes[t[1]])
            else:
                s, e, v = length_symbol(t[1])
                self.code(*lit_codes[s])
                self.bits(v, e)
                s, e, v = distance_symbol(t[2])
                self.code(*dist_codes[s])
                self.bits(v, e)
        self.code(*lit_codes[256])

    def fixed(self, tokens, final=False):
        self.bits(int(final), 1)
        self.bits(1, 2)
        self._tokens(tokens, canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST))

    def dynamic(self, tokens, lit_lengths, dist_lengths, final=False):
        """a dynamic block with these code lengths (len(lit_lengths) >= 257); the lengths are run-length coded greedily as ONE
        sequence, so a run at the end of the literal/length lengths goes on into the distance lengths"""
        assert 257 <= len(lit_lengths) <= 286 and 1 <= len(dist_lengths) <= 30
        seq = list(lit_lengths) + list(dist_lengths)
        ops = []  # (symbol, extra bits, extra value)
        i = 0
        while i < len(seq):
            j = i
            while j < len(seq) and seq[j] == seq[i]:
                j += 1
            run, v = j - i, seq[i]
            if v == 0:
                while run >= 11:
                    n = min(run, 138)
                    ops.append((18, 7, n - 11))
                    run -= n
                if run >= 3:
                    ops.append((17, 3, run - 3))
                    run = 0
                ops += [(0, 0, 0)] * run
            else:
                ops.append((v, 0, 0))
                run -= 1
                while run >= 3:
                    n = min(run, 6)
                    ops.append((16, 2, n - 3))
                    run -= n
                ops += [(v, 0, 0)] * run
            i = j
        used = sorted({o[0] for o in ops})
        if len(used) < 2:
            used = sorted(set(used) | {0, 1})
        clen = complete_lengths(used, 19)
        clen_codes = canonical_codes(clen)
        order = [clen[s] for s in CLEN_ORDER]
        while len(order) > 4 and order[-1] == 0:
            order.pop()
        self.bits(int(final), 1)
        self.bits(2, 2)
        self.bits(len(lit_lengths) - 257, 5)
        self.bits(len(dist_lengths) - 1, 5)
        self.bits(len(order) - 4, 4)
        for v in order:
            self.bits(v, 3)
        for s, e, v in ops:
            self.code(*clen_codes[s])
            self.bits(v, e)
        self.ops = ops
        self._tokens(tokens, canonical_codes(lit_lengths), canonical_codes(dist_lengths))

    def zlib_blocks(self, data, final=False, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
        """what zlib makes of `data` on its own (no history), ended by a sync flush's empty stored block unless final"""
        assert self.aligned
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        self.out += c.compress(data) + c.flush(zlib.Z_FINISH if final else zlib.Z_SYNC_FLUSH)

    def body(self):
        self.align()
        return bytes(self.out)


def zlib_stream(body, raw):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw))
