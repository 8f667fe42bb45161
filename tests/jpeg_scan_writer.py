"""
A baseline JPEG scan writer for the decoder's tests (plain Python and numpy; shares no code with the decoder or its emulator).
write_jpeg turns chosen coefficient blocks and chosen Huffman tables into a 4:2:0 file and logs where every symbol starts, so
that a test has a reference that is independent of the decoder - the coefficients it wrote - and can place codewords, stuffed
bytes and scan ends where the kernels' seams are.
"""
import struct
import typing as T

import numpy as np

from riffusion.util import image_util

ZIGZAG = np.asarray(image_util.JPEG_NATURAL_ORDER)  # zigzag index -> natural (row-major) index


def table_set(tables: T.Sequence[T.Tuple[bytes, bytes]]) -> np.ndarray:
    """(4, 272) uint8 from (BITS, HUFFVAL) of the luma DC, luma AC, chroma DC and chroma AC table"""
    out = np.zeros((4, 272), np.uint8)
    for row, (bits, vals) in zip(out, tables):
        assert len(bits) == 16 and sum(bits) == len(vals) <= 256
        row[:16] = list(bits)
        row[16:16 + len(vals)] = list(vals)
    return out


def annex_k_tables() -> np.ndarray:
    by_class = {tc_th: (bits, vals) for tc_th, bits, vals in image_util.JPEG_HUFFMAN_TABLES}
    return table_set([by_class[k] for k in (0x00, 0x10, 0x01, 0x11)])


def stress_tables() -> np.ndarray:
    """DC: size 11 on a 16-bit code (16 + 11 bits: the longest symbol a baseline scan has).  AC: Annex K's luma lengths - codes
    of 9 and of 10 bits, either side of the decoder's look-up table - with 0x0A and 0xFA (size 10 after a run of 0 and of 15)
    on the last two 16-bit codes, fourteen and fifteen 1-bits each.  The same pair for luma and chroma."""
    dc = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1]), bytes(range(12)))
    bits, vals = next((b, v) for tc_th, b, v in image_util.JPEG_HUFFMAN_TABLES if tc_th == 0x10)
    vals = bytes(v for v in vals if v not in (0x0A, 0xFA)) + bytes([0x0A, 0xFA])
    return table_set([dc, (bits, vals), dc, (bits, vals)])


def ones_tables() -> np.ndarray:
    """complete codes whose last symbol is all 1-bits: DC size 1 on eleven, AC 0x01 on sixteen.  (libjpeg keeps the all-ones
    code free; the decoder's tables do not ask for that.)  A scan of +1 differences and +1 terms is nothing but 0xFF."""
    dc = (bytes([1] * 10 + [2] + [0] * 5), bytes([0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1]))
    ac = (bytes([1] * 15 + [2]), bytes([0x00, 0xF0, 0x0A, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x11, 0x12, 0x21, 0x31, 0xFA, 0x01]))
    return table_set([dc, ac, dc, ac])


def canonical_codes(table: np.ndarray) -> T.Dict[int, T.Tuple[int, int]]:
    """symbol -> (code, length) of one (272,) table, Annex C; raises if BITS is no prefix code"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(table[length - 1])):
            if code >= 1 << length:
                raise ValueError("BITS is no prefix code")
            codes[int(table[16 + k])] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


def _value_bits(v: int, s: int) -> int:
    return v if v >= 0 else v + (1 << s) - 1


class ScanLog(T.NamedTuple):
    """pos[i]: the unstuffed bit position at which symbol i starts; block[i]: its block (scan order); k[i]: the zigzag index the
    decoder is at when it reads it (0: a DC symbol); nbits[i]: code and value bits.  total_bits: the bits coded, before the
    padding; unstuffed: the padded stream; scan: the stream with its stuffed zeros (the file's entropy-coded bytes)."""
    pos: np.ndarray
    block: np.ndarray
    k: np.ndarray
    nbits: np.ndarray
    total_bits: int
    unstuffed: bytes
    scan: bytes


def write_scan(blocks: np.ndarray, huffman: np.ndarray) -> ScanLog:
    blocks = np.asarray(blocks)
    assert blocks.ndim == 2 and blocks.shape[1] == 64 and blocks.shape[0] % 6 == 0
    codes = [canonical_codes(t) for t in huffman]
    pos, blk_log, k_log, n_log = [], [], [], []
    acc, nacc, total = 0, 0, 0
    out = bytearray()

    def put(code_len, value, s, b, k):
        nonlocal acc, nacc, total
        code, length = code_len
        pos.append(total)
        blk_log.append(b)
        k_log.append(k)
        n_log.append(length + s)
        acc = (((acc << length) | code) << s) | value
        nacc += length + s
        total += length + s
        if nacc >= 64:
            keep = nacc & 7
            out.extend((acc >> keep).to_bytes((nacc - keep) // 8, "big"))
            acc &= (1 << keep) - 1
            nacc = keep

    dc_pred = [0, 0, 0]
    for b, row in enumerate(blocks.tolist()):
        comp = 0 if b % 6 < 4 else b % 6 - 3
        dc_t, ac_t = codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3]
        diff = row[0] - dc_pred[comp]
        dc_pred[comp] = row[0]
        s = _size(diff)
        if s > 11:
            raise ValueError(f"block {b}: a DC difference of {diff} is outside baseline")
        put(dc_t[s], _value_bits(diff, s), s, b, 0)
        k, run = 1, 0
        for z in range(1, 64):
            v = row[z]
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(ac_t[0xF0], 0, 0, b, k)
                k += 16
                run -= 16
            s = _size(v)
            if s > 10:
                raise ValueError(f"block {b}: an AC term of {v} is outside baseline")
            put(ac_t[(run << 4) | s], _value_bits(v, s), s, b, k)
            k = z + 1
            run = 0
        if run:
            put(ac_t[0x00], 0, 0, b, k)
    pad = -nacc % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    out.extend(acc.to_bytes((nacc + pad) // 8, "big"))
    unstuffed = bytes(out)
    return ScanLog(np.asarray(pos, np.int64), np.asarray(blk_log, np.int64), np.asarray(k_log, np.int64), np.asarray(n_log, np.int64), total,
                   unstuffed, unstuffed.replace(b"\xff", b"\xff\x00"))


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def write_jpeg(blocks: np.ndarray, H: int, W: int, qtables: np.ndarray, huffman: np.ndarray) -> T.Tuple[bytes, ScanLog]:
    """
    blocks: (6 * mcus, 64) int in scan order - four Y blocks, Cb, Cr per MCU - entry 0 the DC VALUE (the differences per
    component are the writer's), entries 1 .. 63 the AC terms in zigzag order.  qtables: (2, 64) in natural order.  huffman:
    (4, 272) as image_util.jpeg_parse returns it.  -> (the file: SOI, DQT, SOF0 with 2x2 / 1x1 / 1x1 sampling, four DHT, SOS,
    the stuffed scan padded with 1-bits, EOI; the log).  A block whose coefficient 63 is not zero ends without EOB; a run of
    more than 15 zeros is coded with ZRL.  Values outside baseline (a DC difference of more than 11 bits, an AC term of more
    than 10) are refused.
    """
    mcus = ((H + 15) // 16) * ((W + 15) // 16)
    blocks, qtables, huffman = np.asarray(blocks), np.asarray(qtables), np.asarray(huffman, np.uint8)
    assert blocks.shape == (6 * mcus, 64) and qtables.shape == (2, 64) and huffman.shape == (4, 272)
    assert qtables.min() >= 1 and qtables.max() <= 255
    log = write_scan(blocks, huffman)
    parts = [b"\xff\xd8"]
    parts += [_segment(0xDB, bytes([i]) + bytes(int(qtables[i][n]) for n in ZIGZAG)) for i in range(2)]
    parts.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, t in zip((0x00, 0x10, 0x01, 0x11), huffman):
        parts.append(_segment(0xC4, bytes([tc_th]) + t[:16 + int(t[:16].sum())].tobytes()))
    parts.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(parts) + log.scan + b"\xff\xd9", log


def natural_coefficients(blocks: np.ndarray) -> np.ndarray:
    """the (blocks, 64) int16 coefficient buffer a decoder holds for these blocks: natural order, DC as values"""
    out = np.zeros(np.asarray(blocks).shape, np.int16)
    out[:, ZIGZAG] = blocks
    return out


# ---- picture inputs: a float DCT of an RGB tile, quantised ------------------------------------------------------------------------
def _dct_matrix() -> np.ndarray:
    n = np.arange(8)
    m = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m


def picture_blocks(tile: np.ndarray, qtables: np.ndarray) -> np.ndarray:
    """(6 * mcus, 64) blocks of an (H, W, 3) uint8 tile: JFIF's YCbCr in float, edges repeated up to whole MCUs, chroma averaged
    2 x 2, an orthonormal 8 x 8 DCT of the samples - 128, divided by the tables and rounded.  Close to what an encoder writes,
    not equal to any: the decoder under test is compared on the file, not on the tile."""
    tile = np.asarray(tile, np.float64)
    H, W = tile.shape[:2]
    mh, mw = (H + 15) // 16, (W + 15) // 16
    tile = np.pad(tile, ((0, 16 * mh - H), (0, 16 * mw - W), (0, 0)), mode="edge")
    r, g, b = tile[..., 0], tile[..., 1], tile[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b
    cb, cr = (c.reshape(8 * mh, 2, 8 * mw, 2).mean(axis=(1, 3)) for c in (cb, cr))
    d = _dct_matrix()

    def blocks_of(plane, q):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        tiles = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = np.rint(np.einsum("ij,abjk,lk->abil", d, tiles, d) / np.asarray(q, np.float64).reshape(8, 8)).astype(np.int64)
        return coef.reshape(bh, bw, 64)[:, :, ZIGZAG]

    yb, cbb, crb = blocks_of(y, qtables[0]), blocks_of(cb, qtables[1]), blocks_of(cr, qtables[1])
    out = np.zeros((mh, mw, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = yb[k >> 1::2, k & 1::2]
    out[:, :, 4], out[:, :, 5] = cbb, crb
    return out.reshape(-1, 64)
