"""
The inputs of the PNG decoder's tests (TEST INFRASTRUCTURE ONLY), shared by tests/test_png_decode_cpu.py (the host emulator) and
tests/test_gpu_png_decode.py (the device): files Pillow saves, hand-built deflate streams, hand-written filter rows, damaged streams
with the status each must get, and the emulator itself (csrc/rfx_png_dec_core.h compiled for the host with
tests/emu/rfx_png_dec_emu.cpp).  Everything is built once per process.
"""
import ctypes
import functools
import glob
import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

import deflate_writer as dw
import emu_build
from riffusion.util import image_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EMU_SRC = "rfx_png_dec_emu.cpp"
SIZES = [(1, 1), (1, 2), (2, 3), (3, 5), (31, 7), (33, 50), (70, 87)]
BPP = {0: 1, 2: 3, 3: 1, 6: 4}


# ---- the emulator -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-std=c++17"))
    lib.emu_png_dec_workspace_bytes.restype = ctypes.c_int64
    lib.emu_png_dec_workspace_bytes.argtypes = [ctypes.c_int] * 4
    lib.emu_png_dec_inflate_shared_bytes.restype = ctypes.c_int64
    lib.emu_png_dec_unfilter_shared_bytes.restype = ctypes.c_int64
    lib.emu_png_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    return lib


def pack_batch(streams, palettes=None, entries=None):
    n = len(streams)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    data = np.frombuffer(b"".join(streams), np.uint8).copy()
    pal = np.zeros((n, 256, 3), np.uint8) if palettes is None else np.ascontiguousarray(palettes, dtype=np.uint8).reshape(n, 256, 3)
    ent = np.zeros(n, np.int32) if entries is None else np.ascontiguousarray(entries, dtype=np.int32).reshape(n)
    return offsets, data, pal, ent


def emu_decode(streams, H, W, color_type, palettes=None, entries=None):
    """(rgb (N, H, W, 3), status (N)) of the emulator, the signature of Plan.png_decode"""
    lib = emu()
    n = len(streams)
    offsets, data, pal, ent = pack_batch(streams, palettes, entries)
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    rgb = np.zeros((n, H, W, 3), np.uint8)
    status = np.full(n, -1, np.int32)
    ws = np.zeros(max(1, lib.emu_png_dec_workspace_bytes(n, H, W, color_type)), np.uint8)
    rc = lib.emu_png_decode_batch(data.ctypes.data, offsets.ctypes.data, n, H, W, color_type, pal.ctypes.data, ent.ctypes.data, rgb.ctypes.data,
                                  status.ctypes.data, ws.ctypes.data)
    assert rc == 0, rc
    return rgb, status


def case_file_bytes(streams, H, W, color_type, palettes=None, entries=None):
    """the stand-alone emulator program's input file"""
    offsets, data, pal, ent = pack_batch(streams, palettes, entries)
    return struct.pack("<4i", len(streams), H, W, color_type) + offsets.tobytes() + pal.tobytes() + ent.tobytes() + data.tobytes()


def parts_of(data):
    """(info, zlib stream) of a file png_parse gives to the device"""
    info = image_util.png_parse(data)
    assert info.ok_for_device, info.reason
    return info, b"".join(data[a:b] for a, b in info.idat)


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def png_wrap(width, height, color_type, stream, plte=None, extra=b"", depth=8, interlace=0):
    """a PNG file of any colour type around one zlib stream (image_util.png_file writes types 0 and 2 only)"""
    chunk = image_util._png_chunk
    return b"".join((image_util.PNG_SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, 0, 0, interlace)),
                     chunk(b"PLTE", bytes(plte)) if plte is not None else b"", extra, chunk(b"IDAT", bytes(stream)), chunk(b"IEND", b"")))


# ---- contents ---------------------------------------------------------------------------------------------------------------------
def _golden_crop(h, w):
    im = np.asarray(Image.open(os.path.join(GOLDEN, "clip_2_start_103694_ms_duration_5678_ms.png")).convert("RGB"))
    return np.ascontiguousarray(im[100:100 + h, 200:200 + w])


def _random(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _runs(h, w):
    rng = np.random.default_rng(7 * h + w)
    flat = np.repeat(rng.integers(0, 256, h * w * 3 // 5 + 1, dtype=np.uint8), rng.integers(1, 12, h * w * 3 // 5 + 1))[:h * w * 3]
    return np.ascontiguousarray(np.resize(flat, (h, w, 3)))


CONTENTS = {"random": _random, "runs": _runs, "golden": _golden_crop}


def as_mode(rgb, mode):
    im = Image.fromarray(rgb)
    if mode == "L":
        return im.convert("L")
    if mode == "RGBA":
        a = np.dstack([rgb, (rgb.sum(axis=2) % 256).astype(np.uint8)])
        return Image.fromarray(a)
    if mode == "P":  # 8 bits per index: more than 16 colours
        return im.quantize(64) if rgb.shape[0] * rgb.shape[1] > 16 else None
    return im


def pillow_png(im, **kw):
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


SAVE_OPTIONS = {"stored": dict(compress_level=0), "fixed": dict(compress_type=zlib.Z_FIXED), "huffman_only": dict(compress_type=zlib.Z_HUFFMAN_ONLY),
                "rle": dict(compress_type=zlib.Z_RLE), "default": {}, "optimize": dict(optimize=True)}


@functools.lru_cache(maxsize=1)
def pillow_saves():
    """[(name, file)]: every size x mode, the contents and save options rotating so that each option meets each mode, and the
    larger images that give several stored blocks and several pieces of a row"""
    out = []
    options = list(SAVE_OPTIONS.items())
    k = 0
    for si, (h, w) in enumerate(SIZES):
        for mi, mode in enumerate(("L", "RGB", "RGBA", "P")):
            for ci, (cname, make) in enumerate(CONTENTS.items()):
                im = as_mode(make(h, w), mode)
                if im is None or (mode == "P" and im.mode != "P"):
                    continue
                for oi in range(2):
                    oname, kw = options[(k + oi * 3) % len(options)]
                    out.append((f"{cname}_{h}x{w}_{mode}_{oname}", pillow_png(im, **kw)))
                k += 1
    out.append(("random_90x250_RGB_stored", pillow_png(Image.fromarray(_random(90, 250)), compress_level=0)))  # above 65535 filtered bytes
    out.append(("golden_2x3100_RGBA_default", pillow_png(as_mode(_golden_crop(2, 300).repeat(11, axis=1)[:, :3100], "RGBA"))))  # rows of two pieces
    out.append(("random_3x12289_L_default", pillow_png(Image.fromarray(_random(3, 12289)).convert("L"))))  # one byte into the second piece
    return out


def device_writer_file(stream_of, rgb, mode):
    """a file as png_bytes_from_images writes it, the stream from `stream_of(rgb (1, H, W, 3), mode)` -> (stream, channels)"""
    stream, channels = stream_of(rgb[None], mode)
    return image_util.png_file(rgb.shape[1], rgb.shape[0], channels, stream)


# ---- hand-built streams: one row of grey pixels behind a filter byte 0, so that any bytes are an image ----------------------------------
def _one_row_file(body, raw):
    assert raw[0] == 0 and len(raw) >= 2, (raw[0], len(raw))
    return image_util.png_file(len(raw) - 1, 1, 1, dw.zlib_stream(body, raw))


def _literals(n, seed):
    return [dw.lit(b) for b in np.random.default_rng(seed).integers(0, 256, n)]


@functools.lru_cache(maxsize=1)
def hand_built():
    """[(name, file)]"""
    out = []

    def one_fixed(name, tokens):
        w = dw.DeflateWriter()
        w.fixed(tokens, final=True)
        out.append((name, _one_row_file(w.body(), dw.expand(tokens))))

    # every match length, at distances that change with it
    tokens = [dw.lit(0)] + _literals(300, 1)
    for n in range(3, 259):
        tokens.append(dw.match(n, 1 + (n * 7) % 250))
    one_fixed("every_length", tokens)
    # distances: 1, below the length without dividing it, the length itself
    tokens = [dw.lit(0)] + _literals(100, 2) + [dw.match(50, 1), dw.match(100, 7), dw.match(258, 100), dw.match(64, 64), dw.match(3, 2), dw.match(258, 257)]
    one_fixed("short_distances", tokens)
    # distance 32768 exactly, and matches across the ring's wrap (position 32768)
    tokens = [dw.lit(0)] + _literals(255, 3)
    made = 256
    while made < 32768 - 600:
        tokens.append(dw.match(258, 251))
        made += 258
    tokens += _literals(32768 - 100 - made, 4)
    tokens += [dw.match(258, 5), dw.match(258, 32768 - 90), dw.match(100, 32768), dw.match(258, 32768), dw.match(258, 32767), dw.match(3, 32768),
               dw.match(200, 3), dw.match(258, 32768 - 257), dw.match(258, 32768 - 30)]
    one_fixed("far_distances_and_ring_wrap", tokens)
    # blocks: an empty stored block between coded blocks (zlib's sync flush), a stored block behind a block that ends inside a
    # byte, a final empty fixed block
    raw_a = b"\x00" + bytes(np.random.default_rng(5).integers(0, 8, 3000, dtype=np.uint8))
    raw_b = bytes(np.random.default_rng(6).integers(0, 256, 500, dtype=np.uint8))
    toks = _literals(11, 7) + [dw.match(30, 11)]
    w = dw.DeflateWriter()
    w.zlib_blocks(raw_a)  # dynamic blocks, then 00 00 FF FF
    w.fixed(toks)
    assert not w.aligned
    w.stored(raw_b)
    w.zlib_blocks(raw_b[:100], level=1)
    w.stored(b"")
    w.fixed([], final=True)
    out.append(("block_kinds", _one_row_file(w.body(), raw_a + dw.expand(toks, raw_a) + raw_b + raw_b[:100])))
    # a dynamic header whose run of zeros goes from the literal/length lengths into the distance lengths
    used = list(range(0, 40)) + [256, 257, 258, 259, 260]
    lit_lengths = dw.complete_lengths(used, 286)
    dist_lengths = [0, 0, 0, 0, 1, 1]  # distances 5 .. 8
    toks = [dw.lit(0)] + [dw.lit(b % 40) for b in range(200)] + [dw.match(5, 5), dw.match(6, 7), dw.match(4, 8)] + [dw.lit(39)]
    w = dw.DeflateWriter()
    w.dynamic(toks, lit_lengths, dist_lengths, final=True)
    assert (18, 7, 25 + 4 - 11) in w.ops, "one run of zeros: the 25 last literal/length lengths and the 4 first distance lengths"
    out.append(("repeat_crosses_into_distances", _one_row_file(w.body(), dw.expand(toks))))
    # a distance code of a single one-bit code
    w = dw.DeflateWriter()
    toks = [dw.lit(0)] + [dw.lit(b % 40) for b in range(50)] + [dw.match(6, 1), dw.match(3, 1), dw.match(5, 1)]
    w.dynamic(toks, lit_lengths, [1], final=True)
    out.append(("single_distance_code", _one_row_file(w.body(), dw.expand(toks))))
    return out


# ---- filters: filtered bytes written here, the pixels are Pillow's of the same file -------------------------------------------------
@functools.lru_cache(maxsize=1)
def filter_files():
    """[(name, file)]: each filter type in row 0 and below, at every bpp"""
    out = []
    rng = np.random.default_rng(11)
    for color_type, bpp in ((0, 1), (2, 3), (6, 4)):
        w = 9
        for first in range(5):
            rows = []
            for y, t in enumerate([first, 4, 3, 1, 2, 0, 4, 3]):
                rows.append(bytes([t]) + bytes(rng.integers(0, 256, w * bpp, dtype=np.uint8)))
            out.append((f"type{color_type}_first_row_filter_{first}", png_wrap(w, len(rows), color_type, zlib.compress(b"".join(rows)))))
    # Paeth's ties on grey, (left, up, upper-left): x = 1 (25, 10, 20) pb = pc < pa -> up; x = 3 (10, 25, 20) pa = pc < pb -> left;
    # x = 4 (10, 10, 25) pa = pb < pc -> left; x = 5 (10, 10, 10) all equal -> left.  Row 2: an Average whose sum (0 + 25) is odd.
    rows = [bytes([0, 20, 10, 20, 25, 10, 10]), bytes([4, 5, 0, 246, 0, 0, 0]), bytes([3, 1, 2, 3, 4, 5, 6])]
    out.append(("paeth_ties_and_odd_average", png_wrap(6, len(rows), 0, zlib.compress(b"".join(rows)))))
    return out


# ---- damaged streams ------------------------------------------------------------------------------------------------------------------
DAMAGE_H, DAMAGE_W = 3, 5  # RGB


@functools.lru_cache(maxsize=1)
def damaged():
    """[(name, stream, expected status)] for a 3 x 5 RGB image, each a minimal edit of a good stream"""
    rng = np.random.default_rng(21)
    raw = b"".join(bytes([t]) + bytes(rng.integers(0, 256, DAMAGE_W * 3, dtype=np.uint8)) for t in (1, 4, 2))
    good = zlib.compress(raw)
    out = [("good", good, 0)]
    out += [(f"truncated_at_{k}", good[:k], 6) for k in range(len(good))]
    out.append(("adler_flipped", good[:-2] + bytes([good[-2] ^ 0x10]) + good[-1:], 9))
    out.append(("zlib_check_bits", b"\x78\x9d" + good[2:], 1))
    out.append(("zlib_method", b"\x79\x9c" + good[2:], 1))
    out.append(("zlib_preset_dictionary", b"\x78\xbb" + good[2:], 1))
    out.append(("left_over_byte", good + b"\x00", 10))
    out.append(("one_byte_too_much", zlib.compress(raw + b"\x00"), 7))
    out.append(("one_byte_too_little", zlib.compress(raw[:-1]), 8))
    out.append(("block_type_3", b"\x78\x9c\x07" + good[3:], 2))
    w = dw.DeflateWriter()
    w.stored(raw, final=True, nlen=(len(raw) ^ 0xFFFF) ^ 0x0100)
    out.append(("nlen_wrong", dw.zlib_stream(w.body(), raw), 2))
    w = dw.DeflateWriter()
    w.fixed([dw.lit(0), dw.lit(9), dw.match(3, 3)], final=True)
    out.append(("distance_one_past_the_start", dw.zlib_stream(w.body(), raw), 5))
    w = dw.DeflateWriter()
    w.fixed([dw.lit(0), ("sym", 286)], final=True)
    out.append(("length_symbol_286", dw.zlib_stream(w.body(), raw), 4))
    w = dw.DeflateWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)  # nineteen codes of one bit
    out.append(("over_subscribed_header", dw.zlib_stream(w.body() + bytes(8), raw), 3))
    bad_filter = bytearray(raw)
    bad_filter[DAMAGE_W * 3 + 1] = 5
    out.append(("filter_byte_5", zlib.compress(bytes(bad_filter)), 11))
    return out


def palette_damage():
    """(file, stream, palette (256, 3), entries): a 2 x 3 palette image with a pixel whose index is the entry count -> status 12"""
    plte = bytes(range(12))
    raw = bytes([0, 0, 1, 2]) + bytes([0, 3, 4, 1])
    stream = zlib.compress(raw)
    pal = np.zeros((256, 3), np.uint8)
    pal[:4] = np.frombuffer(plte, np.uint8).reshape(4, 3)
    return png_wrap(3, 2, 3, stream, plte=plte), stream, pal, 4


def damaged_file(stream):
    return image_util.png_file(DAMAGE_W, DAMAGE_H, 3, stream)


def golden_files():
    return [(os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(GOLDEN, "*.png")))]


def decode_files(decode, files):
    """{name: (status, pixels)} of files through `decode(streams, H, W, color_type, palettes, entries)`, one call per (size, colour type)"""
    groups, result = {}, {}
    for name, data in files:
        info, stream = parts_of(data)
        groups.setdefault((info.height, info.width, info.color_type), []).append((name, info, stream))
    for (H, W, ct), members in groups.items():
        rgb, status = decode([m[2] for m in members], H, W, ct, np.stack([m[1].palette for m in members]),
                             np.array([m[1].palette_entries for m in members], np.int32))
        rgb = np.asarray(rgb.cpu()) if hasattr(rgb, "cpu") else rgb
        for j, m in enumerate(members):
            result[m[0]] = (int(status[j]), rgb[j])
    return result


def host_only_files():
    """(a 16-bit RGB file, an interlaced file - one pixel: Adam7's first pass is the image -, a JPEG): files png_parse keeps on the host"""
    rng = np.random.default_rng(31)
    rows = b"".join(bytes([0]) + bytes(rng.integers(0, 256, 4 * 6, dtype=np.uint8)) for _ in range(3))
    buf = io.BytesIO()
    Image.fromarray(_random(16, 16)).save(buf, "JPEG")
    return png_wrap(4, 3, 2, zlib.compress(rows), depth=16), png_wrap(1, 1, 2, zlib.compress(bytes([0, 9, 8, 7])), interlace=1), buf.getvalue()
