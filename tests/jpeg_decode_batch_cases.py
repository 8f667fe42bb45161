"""
The cases of the JPEG decoder's packed batch (TEST INFRASTRUCTURE ONLY), shared by tests/test_jpeg_decode_batch_cpu.py (the host
emulator) and tests/test_gpu_jpeg_decode_seams.py and tests/test_gpu_jpeg_decode_large.py (the device): files from
tests/jpeg_scan_writer.py whose codewords, stuffed bytes and scan ends fall on the seams of the kernels, the large cases L1-L6, the
emulator's batch entry and the check of a workspace's stages against what the writer wrote.
"""
import ctypes
import functools
import os
import subprocess
import typing as T

import numpy as np

import jpeg_scan_writer as jw
from jpeg_cases import CONTENTS, STEREO_PNG, _golden, _random
from jpeg_decode_cases import DAMAGE_TILES, SMALL, _emu, _sanitizer_program, damaged_scans, pillow_jpeg
from riffusion import _hip
from riffusion.util import image_util


# ---- the emulator's batch entry ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def emu():
    lib = _emu()
    lib.emu_jpeg_dec_layout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    lib.emu_jpeg_dec_layout.restype = None
    for f in (lib.emu_jpeg_dec_region_offset, lib.emu_jpeg_dec_chunk_offset):
        f.argtypes, f.restype = [ctypes.c_int64] * 3, ctypes.c_int64
    lib.emu_jpeg_dec_unstuff_trip_chunks.restype = ctypes.c_int
    lib.emu_jpeg_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
    return lib


def sub_bits():
    return emu().emu_jpeg_dec_sub_bits()


def group_bits():
    return emu().emu_jpeg_dec_group() * sub_bits()


class Layout(T.NamedTuple):
    unstuffed: int
    pre: int
    ulen: int
    coef: int
    planes: int
    total: int
    coef_bytes: int


def layout(N, H, W, total_scan_bytes):
    out = np.zeros(7, np.int64)
    emu().emu_jpeg_dec_layout(N, H, W, total_scan_bytes, out.ctypes.data)
    return Layout(*(int(v) for v in out))


class Case(T.NamedTuple):
    """one call of the entry.  blocks[n]: what the writer coded (None: a Pillow file or no scan); unstuffed[n]: the writer's
    stream (None: not known); files[n]: the whole file when Pillow is the reference of its pixels, else None (the emulator is)."""
    name: str
    H: int
    W: int
    scans: T.List[bytes]
    blocks: T.List[T.Optional[np.ndarray]]
    unstuffed: T.List[T.Optional[bytes]]
    files: T.List[T.Optional[bytes]]
    qtables: np.ndarray
    huffman: np.ndarray
    off0: int
    status: T.List[int]

    @property
    def offsets(self):
        return np.cumsum([self.off0] + [len(s) for s in self.scans]).astype(np.int64)

    def buffer(self, tail=0):
        """the scans back to back behind off0 bytes of 0xFF; `tail` bytes of 0x00 after offsets[N]"""
        return b"\xff" * self.off0 + b"".join(self.scans) + b"\0" * tail


class Image(T.NamedTuple):
    scan: bytes
    blocks: T.Optional[np.ndarray]
    unstuffed: T.Optional[bytes]
    file: T.Optional[bytes]
    qtables: np.ndarray
    huffman: np.ndarray
    status: int = 0


def case(name, H, W, images, off0=0):
    return Case(name, H, W, [i.scan for i in images], [i.blocks for i in images], [i.unstuffed for i in images], [i.file for i in images],
                np.stack([i.qtables for i in images]).astype(np.uint16), np.stack([i.huffman for i in images]).astype(np.uint8), off0,
                [i.status for i in images])


Q75 = functools.lru_cache(maxsize=None)(lambda: _hip.jpeg_quant_tables(75))
ANNEX_K, STRESS, ONES = jw.annex_k_tables(), jw.stress_tables(), jw.ones_tables()
# the stress images' quantisation tables: all 1, which keeps jpeg_idct_islow's 32-bit sums of 63 terms of 1023 from overflowing
# (with a picture's tables they would: libjpeg lets them wrap, the host emulator under a sanitizer must not)
QONE = np.ones((2, 64), np.uint16)


def written(blocks, H, W, huffman, picture=False, qtables=None):
    """an image from the writer; picture: Pillow decodes the file and is the reference of its pixels"""
    if qtables is None:
        qtables = QONE if huffman is not ANNEX_K else Q75()
    data, log = jw.write_jpeg(blocks, H, W, qtables, huffman)
    return Image(log.scan, np.asarray(blocks), log.unstuffed, data if picture else None, qtables, huffman), log


def pillow_image(data):
    info = image_util.jpeg_parse(data)
    assert info.ok_for_device, info.reason
    return Image(data[info.scan[0]:info.scan[1]], None, None, data, info.qtables, info.huffman)


def mcus_of(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


def stress_blocks(H, W, size=10):
    """every AC term the largest of `size` bits (value bits all 1), DC values 1023 / -1024 in turn per component: differences
    of +-2047, size 11"""
    blocks = np.full((6 * mcus_of(H, W), 64), (1 << size) - 1, np.int64)
    turn = np.zeros(3, np.int64)
    for b in range(len(blocks)):
        comp = 0 if b % 6 < 4 else b % 6 - 3
        blocks[b, 0] = -1024 if turn[comp] & 1 else 1023
        turn[comp] += 1
    return blocks


def steer(blocks, huffman, targets, pick):
    """Moves symbols onto chosen bit positions.  For every target in turn: pick(log, target) names a symbol that starts at or
    after it; as many 26-bit AC symbols before that one as it is bits late (size 10 after a run of 0 in the stress tables)
    become 25-bit ones (size 9), each of which brings it one bit forward.  Returns the log of the final scan."""
    blocks, floor = blocks, -1
    for target in targets:
        log = jw.write_scan(blocks, huffman)
        i = pick(log, target)
        late, j = int(log.pos[i] - target), i
        assert late >= 0, late
        while late:
            j -= 1
            assert j >= 0 and log.pos[j] > floor, "not enough symbols to shorten"
            if log.k[j] > 0 and log.nbits[j] == 26:
                blocks[log.block[j], log.k[j]] = 511
                late -= 1
        floor = target
    return jw.write_scan(blocks, huffman)


def first_long_ac(log, target):
    return int(np.flatnonzero((log.pos >= target) & (log.k >= 1) & (log.k <= 60) & (log.nbits == 26))[0])


def state_at(log, bit):
    """(block of the MCU, zigzag index) of the first symbol that starts at or after `bit`: the state a subsequence that starts
    at `bit` is decoded from"""
    i = int(np.searchsorted(log.pos, bit))
    return int(log.block[i] % 6), int(log.k[i])


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def e1_eob_only():
    H = W = 512
    img, log = written(np.zeros((6 * mcus_of(H, W), 64), np.int64), H, W, ANNEX_K)
    S = sub_bits()
    starts = dict(zip(log.pos.tolist(), zip((log.block % 6).tolist(), log.k.tolist())))
    assert log.total_bits == 32 * 1024 and all(starts[p] == (0, 0) for p in range(0, log.total_bits, S))  # every subsequence starts an MCU
    assert S % 32 == 0, S % 32  # ... and holds S / 32 MCUs of six blocks: the block counts the scan adds up
    return case("E1", H, W, [img])


def e2_long_blocks():
    H, W = 64, 160
    img, log = written(stress_blocks(H, W), H, W, STRESS)
    S = sub_bits()
    ends = log.pos[np.flatnonzero(np.diff(log.block))] // S  # the subsequence in which each block's last symbol starts
    nsub = -(-log.total_bits // S)
    assert len(set(range(nsub)) - set(ends.tolist()) - {nsub - 1}) > 0, (nsub, ends)  # a subsequence without a block end
    assert any(min(state_at(log, i * S)) > 0 for i in range(1, nsub))  # a boundary state with k != 0 and blk != 0
    return case("E2", H, W, [img])


def e3_group_seam(variant):
    H, W = 64, 304
    G = group_bits()
    at = {"starts_at_G-1": G - 1, "ends_at_G": G, "starts_at_G-27": G - 27}[variant]
    blocks = stress_blocks(H, W)
    log = steer(blocks, STRESS, [at, at + G], first_long_ac)
    assert log.total_bits > 2 * G, (log.total_bits, 2 * G)  # three groups
    for seam in (G, 2 * G):
        i = int(np.flatnonzero(log.pos == seam + at - G)[0])  # a symbol starts there
        if variant != "ends_at_G":
            assert log.nbits[i] == 26, log.nbits[i]
        assert state_at(log, seam)[1] != 0, (seam, state_at(log, seam))  # the carried state is inside a block
    img, log2 = written(blocks, H, W, STRESS)
    assert log2.scan == log.scan, (log2.scan, log.scan)
    return case("E3_" + variant, H, W, [img])


def e4_tail(variant):
    S, G = sub_bits(), group_bits()
    H, W = (16, 432) if variant == "multiple_of_G" else (16, 48)
    blocks = stress_blocks(H, W)
    unit = G if variant == "multiple_of_G" else S
    last = lambda log, target: len(log.pos) - 1  # noqa: E731
    natural = jw.write_scan(blocks, STRESS)
    # the last symbol (26 bits): 10 bits before a multiple of the unit (16 bits behind it), or 26 bits before (none)
    back = 10 if variant == "short_tail" else 26
    target = int(natural.pos[-1] + back) // unit * unit - back
    log = steer(blocks, STRESS, [target], last)
    bits = 8 * len(log.unstuffed)
    if variant == "short_tail":
        assert 1 <= bits % S <= 26 and log.pos[-1] < bits // S * S, (bits % S, log.pos[-1], bits // S * S)  # nothing starts in the last subsequence
    else:
        assert bits % unit == 0 and bits == log.total_bits, (bits % unit, bits, log.total_bits)
    img, _ = written(blocks, H, W, STRESS)
    return case("E4_" + variant, H, W, [img])


def e5_runs():
    H = W = 32
    rng = np.random.default_rng(55)
    images = []
    for huffman in (ANNEX_K, STRESS):
        blocks = np.zeros((6 * mcus_of(H, W), 64), np.int64)
        blocks[:, 0] = rng.integers(-40, 40, len(blocks))
        for b in range(len(blocks)):
            kind = b % 6
            if kind == 0:
                blocks[b, 63] = rng.choice([-3, 1, 100])  # the only AC term: coefficient 63, after three ZRL and a run of 14
            elif kind == 1:
                blocks[b, 1:] = rng.integers(1, 30, 63) * rng.choice([-1, 1], 63)  # every term coded: ends at 63 without EOB
            elif kind in (2, 3, 4):
                blocks[b, 16 * (kind - 1)] = rng.choice([-1, 5, -200])  # a lone term at 16, 32, 48
        img, log = written(blocks, H, W, huffman, qtables=QONE)
        sym = lambda i: (int(log.block[i]), int(log.k[i]))  # noqa: E731
        syms = [sym(i) for i in range(len(log.pos))]
        assert [s for s in syms if s[0] == 0] == [(0, 0), (0, 1), (0, 17), (0, 33), (0, 49)]  # DC, ZRL x 3, 14 / size: no EOB
        assert [s for s in syms if s[0] == 1][-1] == (1, 63) and syms[syms.index((1, 63)) + 1] == (2, 0)  # ... then the next DC
        assert [s for s in syms if s[0] == 3] == [(3, 0), (3, 1), (3, 17), (3, 33)]  # DC, ZRL, 15 / size at 32, EOB
        images.append(img)
    return case("E5", H, W, images)


def e6_dc_extremes():
    H = W = 32
    blocks = np.zeros((6 * mcus_of(H, W), 64), np.int64)
    for rows in (np.arange(len(blocks)) % 6 < 4, np.arange(len(blocks)) % 6 == 4, np.arange(len(blocks)) % 6 == 5):
        blocks[rows, 0] = 2047 * (1 - np.arange(rows.sum()) % 2)  # 2047, 0, 2047, ... per component: differences of +2047 / -2047
    img, log = written(blocks, H, W, STRESS)
    assert (log.nbits[log.k == 0] == 27).all(), log.nbits[log.k == 0]  # a 16-bit code and 11 value bits, every block
    return case("E6", H, W, [img])


def _picture(tile, huffman=None):
    tile = np.ascontiguousarray(tile)
    img, _ = written(jw.picture_blocks(tile, Q75()), tile.shape[0], tile.shape[1], ANNEX_K if huffman is None else huffman, picture=True)
    return img


def e7_mixed_tables():
    H, W = 64, 96
    crop = _golden(STEREO_PNG)[200:200 + H, 300:300 + W]
    stress, _ = written(stress_blocks(H, W), H, W, STRESS)
    optimised = pillow_image(pillow_jpeg(crop[::-1], 75, optimize=True))
    assert optimised.huffman.tobytes() not in (ANNEX_K.tobytes(), STRESS.tobytes())
    return case("E7", H, W, [_picture(crop), stress, optimised])


def u1_pair_on_a_chunk_seam(pattern):
    H, W = 16, 48
    img, log = written(stress_blocks(H, W), H, W, STRESS)
    want = {"FF|00": b"\xff\x00", "FF00|FF00": b"\xff\x00\xff\x00"}[pattern]
    i = img.scan.index(want, 16)
    off0 = (15 - i) % 16 if pattern == "FF|00" else (14 - i) % 16
    c = case("U1_" + pattern, H, W, [img], off0)
    buf = c.buffer()
    seam = (off0 + i + 15) // 16 * 16
    if pattern == "FF|00":
        assert buf[seam - 1] == 0xFF and buf[seam] == 0, (buf[seam - 1], buf[seam])
    else:
        assert buf[seam - 2:seam + 2] == b"\xff\x00\xff\x00", buf[seam - 2:seam + 2]
    return c


def u2_pass_seam():
    H, W = 32, 96
    chunk, per_pass = 16, emu().emu_jpeg_dec_scan_threads()
    seam = chunk * per_pass  # relative to lo & ~15
    for seed in range(64):  # the sizes of the first blocks' terms move the bytes: look for a pair whose 0xFF is the last byte of the first pass
        blocks = stress_blocks(H, W)
        blocks[:12, 1:] = (1 << np.random.default_rng(seed).integers(1, 11, (12, 63))) - 1
        img, log = written(blocks, H, W, STRESS)
        found = [i for i in range(seam - 16, seam - 1) if img.scan[i:i + 2] == b"\xff\x00"]
        if len(img.scan) > seam + 64 and found:
            break
    else:
        raise AssertionError("no seed puts a stuffed pair on the pass seam")
    off0 = seam - 1 - found[-1]
    c = case("U2", H, W, [img], off0)
    buf = c.buffer()
    assert 1 <= off0 <= 15 and buf[seam - 1] == 0xFF and buf[seam] == 0, (off0, buf[seam - 1], buf[seam])  # lo unaligned; the pair straddles the seam
    assert b"\xff\x00" in buf[off0:seam - 1] and b"\xff\x00" in buf[seam + 1:], (buf[off0:seam - 1], buf[seam + 1:])  # ... and stuffed bytes on both sides
    return c


@functools.lru_cache(maxsize=1)
def _abc():
    """16 x 16: A ends FF 00 (its last value bits and the padding are 1s); B begins 00 (luma DC "00", AC 0/1 "00", a 0 value
    bit, twice); C is ordinary"""
    H = W = 16
    a, _ = written(stress_blocks(H, W), H, W, STRESS)
    blocks = np.zeros((6, 64), np.int64)
    blocks[0, 1:9] = -1
    blocks[1:, 0] = [3, -7, 20, 5, -9]
    b, _ = written(blocks, H, W, ANNEX_K)
    c = _picture(_golden(STEREO_PNG)[100:116, 40:56])
    assert a.scan.endswith(b"\xff\x00") and b.scan[0] == 0, (a.scan[-2:], b.scan[0])
    return a, b, c


def u3_neighbours(order, seam_at):
    a, b, c = _abc()
    if order == "A'BC":
        a = a._replace(scan=a.scan[:-1], status=1)  # a dangling 0xFF; the stream without its stuffed zeros is A's
        assert a.scan[-1] == 0xFF, a.scan[-1]
    images = {"ABC": [a, b, c], "BAC": [b, a, c], "A'BC": [a, b, c]}[order]
    end_of_a = sum(len(i.scan) for i in images[:images.index(a) + 1])
    off0 = (seam_at - end_of_a) % 16
    cs = case(f"U3_{order}_{seam_at}", 16, 16, images, off0)
    assert (off0 + end_of_a) % 16 == seam_at, ((off0 + end_of_a) % 16, seam_at)  # A's last byte and its neighbour's first: in one chunk (8) or in two (0)
    return cs


def u4_first_offset(off0):
    a, b, c = _abc()
    tail = a._replace(scan=a.scan[:-1], status=1)  # ends 0xFF: the 0x00 behind offsets[N] is not its stuffed zero
    cs = case(f"U4_{off0}", 16, 16, [b, c, tail], off0)
    buf = cs.buffer(tail=24)
    assert (off0 == 0 or buf[off0 - 1] == 0xFF) and buf[off0] == 0 and buf[cs.offsets[-1] - 1] == 0xFF and buf[cs.offsets[-1]] == 0
    return cs


def u5_empty_scan(where):
    a, b, c = _abc()
    d, _ = written(stress_blocks(16, 16, size=3), 16, 16, STRESS)
    images = [a, b, c, d]
    images.insert(where, Image(b"", None, b"", None, Q75(), ANNEX_K, status=6))
    cs = case(f"U5_{where}", 16, 16, images, 3)
    assert cs.offsets[where] == cs.offsets[where + 1], (cs.offsets[where], cs.offsets[where + 1])
    return cs


def u6_mostly_stuffing():
    H = W = 16
    blocks = np.ones((6, 64), np.int64)
    blocks[:, 0] = [1, 2, 3, 4, 1, 1]  # every difference +1
    img, log = written(blocks, H, W, ONES)
    assert img.scan.count(b"\xff\x00") >= 0.45 * len(img.scan), (img.scan.count(b"\xff\x00"), len(img.scan))
    return case("U6", H, W, [img], 7)


def u7_many_tiny():
    H = W = 8
    rng = np.random.default_rng(77)
    images = []
    for n in range(300):
        blocks = np.zeros((6, 64), np.int64)
        blocks[:4, 0] = n - 150  # a DC of its own: two images swapped show
        if n % 3 == 2:
            blocks[:, 1:1 + n % 4] = rng.integers(-7, 8, (6, n % 4))
        blocks[4:, 0] = rng.integers(-20, 20, 2)
        images.append(written(blocks, H, W, ANNEX_K)[0])
    cs = case("U7", H, W, images, 9)
    sizes, off = np.diff(cs.offsets), cs.offsets
    assert sizes.min() >= 4 and sizes.max() <= 40 and len({i.blocks[0, 0] for i in images}) == 300
    assert any(off[n] // 16 == (off[n + 2] - 1) // 16 for n in range(298))  # two whole images inside one chunk
    assert any(off[n + 1] % 16 and off[n + 1] // 16 == off[n + 3] // 16 for n in range(297))  # a chunk shared by four
    return cs


def d1_dc_passes(W):
    H = 16
    mcus = mcus_of(H, W)
    images = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed * 1000 + W)
        blocks = np.zeros((6 * mcus, 64), np.int64)
        for comp, rows in enumerate((np.arange(6 * mcus) % 6 < 4, np.arange(6 * mcus) % 6 == 4, np.arange(6 * mcus) % 6 == 5)):
            n = int(rows.sum())
            steps = rng.integers(1, 6, n) * rng.choice([-1, 1], n)
            walk = np.zeros(n, np.int64)
            v = 0
            for i, s in enumerate(steps.tolist()):  # a walk that never stands still and stays where samples do not clip
                v = v + s if abs(v + s) <= 50 else v - s
                walk[i] = v
            blocks[rows, 0] = walk
        img, log = written(blocks, H, W, ANNEX_K, picture=True)
        assert mcus > 1024 and (np.diff(blocks[np.arange(6 * mcus) % 6 < 4, 0]) != 0).all() and blocks[0, 0] != 0
        images.append(img)
    assert mcus in (1025, 2049), (mcus, (1025, 2049))
    return case(f"D1_{W}", H, W, images, 5)


def p1_small(h, w):
    return case(f"P1_{h}x{w}", h, w, [pillow_image(pillow_jpeg(_random(h, w), q)) for q in (50, 90)], 1)


BUILDERS = {
    "E1": e1_eob_only,
    "E2": e2_long_blocks,
    **{f"E3_{v}": functools.partial(e3_group_seam, v) for v in ("starts_at_G-1", "ends_at_G", "starts_at_G-27")},
    **{f"E4_{v}": functools.partial(e4_tail, v) for v in ("short_tail", "multiple_of_S", "multiple_of_G")},
    "E5": e5_runs,
    "E6": e6_dc_extremes,
    "E7": e7_mixed_tables,
    **{f"U1_{p}": functools.partial(u1_pair_on_a_chunk_seam, p) for p in ("FF|00", "FF00|FF00")},
    "U2": u2_pass_seam,
    **{f"U3_{o}_{s}": functools.partial(u3_neighbours, o, s) for o in ("ABC", "BAC", "A'BC") for s in (8, 0)},
    **{f"U4_{o}": functools.partial(u4_first_offset, o) for o in (0, 16, 5, 37)},
    **{f"U5_{w}": functools.partial(u5_empty_scan, w) for w in (0, 2, 4)},
    "U6": u6_mostly_stuffing,
    "U7": u7_many_tiny,
    **{f"D1_{w}": functools.partial(d1_dc_passes, w) for w in (16400, 32784)},
    **{f"P1_{h}x{w}": functools.partial(p1_small, h, w) for h, w in SMALL},
}


@functools.lru_cache(maxsize=None)
def build_case(name) -> Case:
    c = BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c


# ---- decoding a case on the host --------------------------------------------------------------------------------------------------
class Decoded(T.NamedTuple):
    status: np.ndarray
    rgb: np.ndarray
    workspace: np.ndarray


def emu_batch(c: Case, fill=0xA5) -> Decoded:
    scans = np.frombuffer(c.buffer(), np.uint8).copy()  # exactly offsets[N] bytes
    off, N = c.offsets, len(c.scans)
    lay = layout(N, c.H, c.W, int(off[-1] - off[0]))
    rgb, status = np.zeros((N, c.H, c.W, 3), np.uint8), np.full(N, -1, np.int32)
    workspace = np.full(lay.total, fill, np.uint8)  # whatever the device's memory held before
    qt, huff = np.ascontiguousarray(c.qtables), np.ascontiguousarray(c.huffman)
    rc = emu().emu_jpeg_decode_batch(scans.ctypes.data, off.ctypes.data, N, c.H, c.W, qt.ctypes.data, huff.ctypes.data, rgb.ctypes.data,
                                     status.ctypes.data, workspace.ctypes.data)
    assert rc == 0, rc
    return Decoded(status, rgb, workspace)


def sanitized_batch(c: Case, tmp_path) -> Decoded:
    off, N = c.offsets, len(c.scans)
    src, dst = os.path.join(tmp_path, "case.bin"), os.path.join(tmp_path, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([N, c.H, c.W], np.int32).tobytes() + off.tobytes() + np.ascontiguousarray(c.qtables).tobytes())
        f.write(np.ascontiguousarray(c.huffman).tobytes() + c.buffer())
    done = subprocess.run([_sanitizer_program(), "batch", src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]  # a sanitizer report ends the program with another code
    assert done.stdout.strip() == "batch 0", done.stdout
    out = np.fromfile(dst, np.uint8)
    pixels = N * c.H * c.W * 3
    return Decoded(out[:4 * N].view(np.int32), out[4 * N:4 * N + pixels].reshape(N, c.H, c.W, 3), out[4 * N + pixels:])


@functools.lru_cache(maxsize=None)
def alone(scan, H, W, qtables, huffman):
    """(status, pixels) of one scan through the single-image emulator"""
    buf, out = np.frombuffer(scan, np.uint8).copy(), np.zeros((H, W, 3), np.uint8)
    qt, huff = np.frombuffer(qtables, np.uint16).copy(), np.frombuffer(huffman, np.uint8).copy()
    return _emu().emu_jpeg_decode_u8(buf.ctypes.data, buf.size, H, W, qt.ctypes.data, huff.ctypes.data, out.ctypes.data, None), out


def check_stages(c: Case, got: Decoded, stages=("unstuffed", "coef"), who="emulator"):
    """the lengths and unstuffed regions, then the coefficients, of a workspace against what the writer wrote"""
    off, N = c.offsets, len(c.scans)
    lay = layout(N, c.H, c.W, int(off[-1] - off[0]))
    ws = np.asarray(got.workspace)
    assert ws.size == lay.total, (ws.size, lay.total)
    if "unstuffed" in stages:
        ulen = ws[lay.ulen:lay.ulen + 4 * N].view(np.uint32)
        for n in range(N):
            if c.unstuffed[n] is None:
                continue
            assert ulen[n] == len(c.unstuffed[n]), f"{c.name}: {who}: unstuff scan stage: ulen[{n}] = {ulen[n]}, written {len(c.unstuffed[n])}"
            at = lay.unstuffed + emu().emu_jpeg_dec_region_offset(int(off[n]), int(off[0]), n)
            assert ws[at:at + ulen[n]].tobytes() == c.unstuffed[n], f"{c.name}: {who}: unstuff stage: the region of image {n} differs"
    if "coef" in stages:
        per = 6 * mcus_of(c.H, c.W) * 64
        coef = ws[lay.coef:lay.coef + lay.coef_bytes].view(np.int16).reshape(N, per)
        for n in range(N):
            if c.blocks[n] is not None and c.status[n] == 0:
                assert np.array_equal(coef[n], jw.natural_coefficients(c.blocks[n]).ravel()), \
                    f"{c.name}: {who}: entropy / DC scan stage: the coefficients of image {n} differ"


# ---- the large cases (tests/test_gpu_jpeg_decode_large.py runs the same ones on the device) ---------------------------------------
# jpd_unstuff_kernel runs min(chunk groups of the call's longest scan, 64) workgroups of 256 threads per image, a 16-byte chunk
# per thread: a scan of more bytes than this sends the threads round their loop a second time
UNSTUFF_TRIP_BYTES = 64 * 256 * 16
MANY_GROUPS = 8  # entropy groups (of 256 subsequences) a long scan must exceed
MAX_SCAN_BYTES = (1 << 28) - 64  # kJpdMaxScanBytes


def subsequences(unstuffed_bytes):
    return -(-8 * unstuffed_bytes // sub_bits())


def reach(c: Case, quiet=False):
    """per image (scan bytes, trips of the copy kernel's grid, entropy groups), printed with the call's chunk groups"""
    longest = max(len(s) for s in c.scans)
    chunk_groups = (longest // 16 + 2 + 255) // 256
    per = []
    for n, scan in enumerate(c.scans):
        unstuffed = c.unstuffed[n] if c.unstuffed[n] is not None else scan.replace(b"\xff\x00", b"\xff")
        chunks = -(-(c.offsets[n + 1] - (c.offsets[n] & ~15)) // 16)
        per.append((len(scan), int(-(-chunks // (min(chunk_groups, 64) * 256))), -(-subsequences(len(unstuffed)) // 256)))
    if not quiet:
        shown = per if len(per) <= 8 else f"{len(per)} images, the largest of each: {tuple(max(v) for v in zip(*per))}"
        print(f"{c.name}: chunk groups of the call {chunk_groups} (the grid takes {min(chunk_groups, 64)});",
              "per image (scan bytes, trips of the copy grid, entropy groups):", shown)
    return per


def assert_long(c: Case, n):
    """image n of the case is a long scan: a second trip of the copy kernel's grid and more than eight entropy groups"""
    assert emu().emu_jpeg_dec_unstuff_trip_chunks() * 16 == UNSTUFF_TRIP_BYTES and emu().emu_jpeg_dec_group() == 256
    scan, unstuffed = c.scans[n], c.unstuffed[n]
    assert len(scan) > 64 * 256 * 16 and subsequences(len(unstuffed)) > 8 * 256, (len(scan), subsequences(len(unstuffed)))
    _, trips, groups = reach(c, quiet=True)[n]
    assert trips >= 2 and groups > MANY_GROUPS, (trips, groups, MANY_GROUPS)
    assert min(len(s) for s in c.scans) < 4096, min(len(s) for s in c.scans)  # ... beside an image that idles through that grid


def sound_pillow_image(data):
    """a Pillow file whose scan is sound: its unstuffed stream is the scan without the zeros behind 0xFF"""
    img = pillow_image(data)
    assert b"\xff" not in img.scan.replace(b"\xff\x00", b"")
    return img._replace(unstuffed=img.scan.replace(b"\xff\x00", b"\xff"))


@functools.lru_cache(maxsize=1)
def _l1_images():
    size = 384
    noise = _random(size, size)
    return size, [sound_pillow_image(pillow_jpeg(noise, 100)), sound_pillow_image(pillow_jpeg(noise, 75)),
                  sound_pillow_image(pillow_jpeg(np.zeros((size, size, 3), np.uint8), 100))]


def l1_long_pillow_scan(where):
    size, images = _l1_images()
    c = case("L1_" + where, size, size, images if where == "first" else images[::-1], 0 if where == "first" else 9)
    assert_long(c, 0 if where == "first" else 2)
    assert len({i.qtables.tobytes() for i in images}) == 2, len({i.qtables.tobytes() for i in images})  # quality 100 and quality 75 in one call
    return c


def l2_long_writer_scan():
    H = W = 240  # the smallest (from 240 x 240 in steps of 16) whose stress scan is longer than one trip of the copy grid
    long_, log = written(stress_blocks(H, W), H, W, STRESS)
    short, _ = written(np.zeros((6 * mcus_of(H, W), 64), np.int64), H, W, ANNEX_K, picture=True)
    c = case("L2", H, W, [short, long_], 5)
    assert_long(c, 1)
    # blocks longer than a subsequence in every group: each group has a subsequence in which no block ends
    S, nsub = sub_bits(), subsequences(len(log.unstuffed))
    ends = set((log.pos[np.flatnonzero(np.diff(log.block))] // S).tolist())
    for first in range(0, nsub, 256):
        assert set(range(first, min(first + 256, nsub - 1))) - ends, first
    return c


L3_PLACES = (0, 31, 63)  # of the damaged scans
L3_QUALITIES = (1, 30, 75, 95, 100)


@functools.lru_cache(maxsize=1)
def l3_sound_images():
    """64 images of 64 x 96: five qualities, standard and optimised tables, three contents, each on a cycle of its own"""
    a = _random(64, 96)
    contents = [a, np.ascontiguousarray(a[::-1, ::-1] ^ 0x5A), np.repeat(a[:, :, :1] // 2, 3, axis=2)]  # test_gpu_jpeg_decode._three
    images = [sound_pillow_image(pillow_jpeg(contents[i % 3], L3_QUALITIES[i % 5], optimize=bool(i % 2))) for i in range(64)]
    assert len({(i.qtables.tobytes(), i.huffman.tobytes(), i.scan) for i in images}) == 30
    assert len({i.huffman.tobytes() for i in images}) > 2 and len({i.qtables.tobytes() for i in images}) == 5
    return images


def l3_sound():
    return case("L3_sound", 64, 96, l3_sound_images(), 0)


def l3_with_damage():
    """places 0, 31 and 63: damaged scans of DAMAGE_TILES' tiles (test_jpeg_decode_cpu.py), with their own tables.  Those tiles
    have other sizes than 64 x 96: the call's size is one more thing that is wrong with them.  status 1 stands for "not 0"."""
    images = list(l3_sound_images())
    picks = (("og_beat", "an all-0xFF tail"), ("random_62x33", "one byte flipped mid-scan"), ("random_32x40", "truncated at a third"))
    for place, (tile, what) in zip(L3_PLACES, picks):
        assert tile in DAMAGE_TILES, (tile, DAMAGE_TILES)
        data = pillow_jpeg(CONTENTS[tile](), DAMAGE_TILES[tile])
        info = image_util.jpeg_parse(data)
        images[place] = Image(damaged_scans(data[info.scan[0]:info.scan[1]])[what], None, None, None, info.qtables, info.huffman, status=1)
    return case("L3", 64, 96, images, 0)


def one_image(c: Case, n) -> Case:
    return Case(f"{c.name}[{n}]", c.H, c.W, [c.scans[n]], [c.blocks[n]], [c.unstuffed[n]], [c.files[n]], c.qtables[n:n + 1], c.huffman[n:n + 1], 0,
                [c.status[n]])


BAD_TABLES = ("over-subscribed", "257_codes")


def bad_table(kind):
    """(16,) BITS no decoder can derive codes from"""
    bits = np.zeros(16, np.uint8)
    if kind == "over-subscribed":
        bits[0] = 3  # three codes of one bit
    else:
        bits[7], bits[8] = 128, 129  # 128 of the 256 codes of 8 bits, 129 of the 256 left of 9: 257 symbols
        code = 0
        for length in range(1, 17):
            code = (code + int(bits[length - 1])) << 1
            assert code <= 2 << length, (code, 2 << length)  # no length over-subscribed
        assert int(bits.sum()) == 257, int(bits.sum())
    return bits


def l4_bad_table(kind, which):
    h, w = 23, 37
    images = [sound_pillow_image(pillow_jpeg(t, q)) for t, q in zip((_random(h, w), _random(h, w)[::-1], _random(h, w) ^ 0x33), (75, 90, 50))]
    huffman = images[1].huffman.copy()
    huffman[which, :16] = bad_table(kind)
    images[1] = images[1]._replace(huffman=huffman, file=None, unstuffed=None, status=2)
    return case(f"L4_{kind}_{which}", h, w, images, 0)


def s1_the_largest_of_several_causes():
    """include/rfx.h: "With several causes the largest is reported."  Scans whose causes are known from how they are made:
    0: a stress scan cut inside a block - it ends inside a block (3) and blocks are missing (6);
    1: a 16 x 16 scan less its last byte, a stuffed zero, as a 32 x 32 image - a dangling 0xFF (1) and blocks missing (6);
    2: a sound scan and a dangling 0xFF (1) with a Huffman table that is no prefix code (2);
    3: a sound picture."""
    H = W = 32
    whole, log = written(stress_blocks(H, W), H, W, STRESS)
    i = int(np.flatnonzero((log.block == 13) & (log.k == 30))[0])  # a symbol in the middle of block 13
    cut = log.unstuffed[:int(log.pos[i]) // 8]
    assert cut[-1] != 0xFF and log.pos[i] // 8 * 8 > log.pos[np.flatnonzero(log.block == 13)[0]]  # no marker; the cut is inside the block
    inside = whole._replace(scan=cut.replace(b"\xff", b"\xff\x00"), blocks=None, unstuffed=cut, status=6)
    a = _abc()[0]
    dangling = a._replace(scan=a.scan[:-1], blocks=None, status=6)
    sound = sound_pillow_image(pillow_jpeg(_random(H, W), 75))
    huffman = sound.huffman.copy()
    huffman[1, :16] = bad_table("over-subscribed")
    both = sound._replace(scan=sound.scan + b"\xff", huffman=huffman, file=None, unstuffed=sound.unstuffed + b"\xff", status=2)
    assert a.scan.endswith(b"\xff\x00") and mcus_of(H, W) > 1
    return case("S1", H, W, [inside, dangling, both, sound], 3)


def emulator_blocks(c: Case, host: Decoded) -> Case:
    """the case with the emulator's coefficients as the reference of the images the writer did not write (Pillow's files: the
    emulator's pixels of them are compared with Pillow's), so that check_stages compares a device's coefficients with them"""
    N = len(c.scans)
    lay = layout(N, c.H, c.W, int(c.offsets[-1] - c.offsets[0]))
    coef = np.asarray(host.workspace)[lay.coef:lay.coef + lay.coef_bytes].view(np.int16).reshape(N, -1, 64)
    return c._replace(blocks=[b if b is not None or c.status[n] != 0 else coef[n][:, jw.ZIGZAG].astype(np.int64) for n, b in enumerate(c.blocks)])


LARGE = {
    "L1_first": functools.partial(l1_long_pillow_scan, "first"),
    "L1_last": functools.partial(l1_long_pillow_scan, "last"),
    "L2": l2_long_writer_scan,
    "S1": s1_the_largest_of_several_causes,
    **{f"L4_{k}_{t}": functools.partial(l4_bad_table, k, t) for k in BAD_TABLES for t in range(4)},
}


@functools.lru_cache(maxsize=None)
def build_large(name) -> Case:
    c = {**LARGE, "L3": l3_with_damage, "L3_sound": l3_sound}[name]()
    assert c.name == name, (c.name, name)
    return c
