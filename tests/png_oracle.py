"""
A plain numpy restatement of the two rules of the device PNG writer that no PNG reader checks (csrc/rfx_png_core.h): which filter
every row gets, and how a block of the filtered stream is cut into literals and distance-1 matches.  Written from the rules, not
from the C++.
"""
import typing as T

import numpy as np

BLOCK_ROWS = 32
# RFC 1951 3.2.5: (symbol, first length, extra bits)
LENGTH_CODES = [(257 + i, 3 + i, 0) for i in range(8)] + [
    (265, 11, 1), (266, 13, 1), (267, 15, 1), (268, 17, 1), (269, 19, 2), (270, 23, 2), (271, 27, 2), (272, 31, 2),
    (273, 35, 3), (274, 43, 3), (275, 51, 3), (276, 59, 3), (277, 67, 4), (278, 83, 4), (279, 99, 4), (280, 115, 4),
    (281, 131, 5), (282, 163, 5), (283, 195, 5), (284, 227, 5), (285, 258, 0)]


def source_rows(tile: np.ndarray, channels: int) -> np.ndarray:
    """(H, W, 3) uint8 -> the (H, W * channels) bytes the file holds: all three channels, or channel 0"""
    tile = np.asarray(tile)
    return tile.reshape(tile.shape[0], -1) if channels == 3 else tile[:, :, 0]


def filtered(tile: np.ndarray, channels: int) -> T.Tuple[bytes, np.ndarray]:
    """(the filtered stream zlib.decompress must give back, each row's filter type): every row gets the one of None, Sub, Up,
    Average, Paeth whose filtered bytes, read as int8, have the least sum of absolute values; the first of equals"""
    x = source_rows(tile, channels).astype(np.int64)
    H, n = x.shape
    a = np.zeros_like(x)
    a[:, channels:] = x[:, :-channels]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, channels:] = x[:-1, :-channels]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255  # (5, H, n)
    cost = np.where(cands < 128, cands, 256 - cands).sum(axis=2)  # (5, H)
    types = np.argmin(cost, axis=0)
    rows = cands[types, np.arange(H)]
    out = np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)
    return out.tobytes(), types


def runs(data: bytes) -> T.List[T.Tuple[int, int]]:
    """the maximal runs of equal bytes: (value, length)"""
    d = np.frombuffer(data, np.uint8)
    if d.size == 0:
        return []
    cuts = np.flatnonzero(np.diff(d.astype(np.int16)) != 0) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [d.size]])
    return [(int(d[s]), int(e - s)) for s, e in zip(starts, ends)]


def tokens(block: bytes) -> T.List[T.Tuple[str, int]]:
    """one block's tokens: ("lit", value) and ("match", length), every match at distance 1"""
    out: T.List[T.Tuple[str, int]] = []
    for value, length in runs(block):
        out.append(("lit", value))
        left = length - 1
        while left >= 3:
            take = min(258, left)
            out.append(("match", take))
            left -= take
        out.extend([("lit", value)] * left)
    return out


def length_symbol(length: int) -> int:
    return max(sym for sym, first, _ in LENGTH_CODES if first <= length)


def histogram(block: bytes) -> np.ndarray:
    """counts of the 286 literal/length symbols of one block's tokens (without the end-of-block)"""
    hist = np.zeros(286, np.int64)
    for kind, v in tokens(block):
        hist[v if kind == "lit" else length_symbol(v)] += 1
    return hist


def blocks(stream: bytes, row_bytes: int) -> T.List[bytes]:
    """the filtered stream cut every BLOCK_ROWS rows"""
    step = BLOCK_ROWS * row_bytes
    return [stream[at:at + step] for at in range(0, len(stream), step)]
