"""
CPU checks of the device PNG writer's stream (csrc/rfx_png_core.h, compiled for the host with tests/emu/rfx_png_emu.cpp, in the
kernels' stages) and of image_util.png_file.  The stream is not zlib's, so nothing is compared with Pillow's IDAT; what is checked
is what a lossless format promises and what the stream states about itself:
  * Pillow reopens every file to the tile's pixels in the expected mode, and to the EXIF that went in;
  * every chunk but IDAT equals the chunk of Pillow's own save of that image; every chunk's CRC is right (the IDAT's comes from the
    emulator's piecewise CRC); zlib inflates the payload (so the piecewise Adler-32 is right) to the filtered bytes
    tests/png_oracle.py works out from the rule (so the filter choice is pinned), and the token histogram of a block is the one the
    oracle derives from the run rule;
  * the code builder alone: lengths within the limit and Kraft sum exactly 1 on histograms whose unlimited Huffman depth passes it;
  * the file is at most 1.02 x Pillow's save(..., compress_type=zlib.Z_RLE) of the same pixels in the same mode, on every
    spectrogram golden tile;
  * the capacity is never passed; refusals.
"""
import ctypes
import functools
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_oracle
from riffusion import _hip
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MONO_PNG = "clip_2_start_103694_ms_duration_5678_ms.png"
STEREO_PNG = "clip_2_start_103694_ms_duration_5678_ms_stereo.png"
# (H, W): one row; a last block of 1 row (33) and of 31 rows (31); row lengths of every residue mod 4
SIZES = [(1, 1), (1, 2), (3, 5), (31, 7), (32, 8), (33, 50), (65, 171), (70, 87)]
RUN_LENGTHS = (3, 4, 257, 258, 259, 260, 261, 262, 517)
SPECTROGRAM_TILES = ("agile.png", "marim.png", "motorway.png", "vibes.png", "og_beat.png", MONO_PNG, STEREO_PNG)
MASKS = ("mask_beat_lines_80.png", "mask_gradient_dark.png")
RATIO_BOUND = 1.02


def _golden(name):
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB")))


def _random(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _mono(grey):
    return np.ascontiguousarray(np.repeat(np.asarray(grey, np.uint8)[:, :, None], 3, axis=2))


def _run_heavy(h, w):
    """few values in long stretches, colour: runs of every length up to whole rows, many of them across row ends"""
    rng = np.random.default_rng(7000 * h + w)
    flat = np.repeat(rng.integers(0, 4, size=h * w * 3 // 2 + 1), rng.integers(1, 12, size=h * w * 3 // 2 + 1))[:h * w * 3]
    return np.ascontiguousarray((flat * 85).astype(np.uint8).reshape(h, w, 3))


def _run_lengths_tile():
    """A grey tile whose rows are 1, 255, 1, 255, ... (a row and the next out of step), so that filter None wins every row, with
    stretches of zeros: rows 0 .. 8 hold one run each of exactly RUN_LENGTHS bytes; row 10 ends and row 11 begins with zeros (a run
    across a row end, through the filter byte 0); row 31 ends and row 32 begins with zeros (a run cut at the block's end)."""
    H, W = 40, 600
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.where((yy + xx) & 1, 255, 1).astype(np.uint8)
    for row, n in enumerate(RUN_LENGTHS):
        g[row, 20:20 + n] = 0
    g[10, W - 7:] = 0
    g[11, :5] = 0
    g[31, W - 9:] = 0
    g[32, :11] = 0
    return _mono(g)


CONTENTS = {
    **{f"random_{h}x{w}": functools.partial(_random, h, w) for h, w in SIZES},
    **{f"runs_{h}x{w}": functools.partial(_run_heavy, h, w) for h, w in SIZES},
    "zeros": lambda: np.zeros((70, 87, 3), np.uint8),
    "ones": lambda: np.full((33, 50, 3), 255, np.uint8),
    "mono_noise": lambda: _mono(np.random.default_rng(5).integers(0, 256, size=(65, 171), dtype=np.uint8)),
    "run_lengths": _run_lengths_tile,
    **{name: functools.partial(_golden, name) for name in SPECTROGRAM_TILES + MASKS},
}


def is_mono(tile):
    return bool((tile[:, :, 0] == tile[:, :, 1]).all() and (tile[:, :, 0] == tile[:, :, 2]).all())


@functools.lru_cache(maxsize=None)
def _tile(name):
    t = CONTENTS[name]()
    t.setflags(write=False)
    return t


def modes_of(name):
    return ("rgb", "gray", "auto") if is_mono(_tile(name)) else ("rgb", "auto")


CASES = [(name, mode) for name in CONTENTS for mode in modes_of(name)]


@functools.lru_cache(maxsize=1)
def _emu():
    import tempfile

    so = os.path.join(tempfile.mkdtemp(prefix="png_emu"), "librfx_png_emu.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "emu", "rfx_png_emu.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.emu_png_stream_capacity.restype = ctypes.c_uint64
    lib.emu_png_stream_capacity.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.emu_png_code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_png_block_histogram.restype = None
    lib.emu_png_block_histogram.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.emu_png_encode_u8.restype = ctypes.c_int64
    lib.emu_png_encode_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emu_stream(tile, mode):
    """the emulator's (stream, CRC-32 of b"IDAT" + stream, channels, [blocks without a match, longest code, blocks limited])"""
    lib = _emu()
    tile = np.ascontiguousarray(tile, dtype=np.uint8)
    H, W, _ = tile.shape
    m = _hip.PNG_MODES[mode]
    cap = lib.emu_png_stream_capacity(H, W, 1 if m == 1 else 3)
    out = np.zeros(cap, np.uint8)
    crc, ch = ctypes.c_uint32(0), ctypes.c_int32(-1)
    stats = np.zeros(3, np.int64)
    n = lib.emu_png_encode_u8(tile.ctypes.data, H, W, m, out.ctypes.data, cap, ctypes.byref(crc), ctypes.byref(ch), stats.ctypes.data)
    assert 0 <= n <= cap, n  # (-1: the capacity would be passed)
    return out[:n].tobytes(), int(crc.value), int(ch.value), stats


def emu_file(tile, mode, exif=None):
    stream, crc, ch, _ = emu_stream(tile, mode)
    assert ch in (1, 3)
    return image_util.png_file(tile.shape[1], tile.shape[0], ch, stream, crc, image_util.png_exif_bytes(exif))


def pillow_image(tile, channels):
    return Image.fromarray(np.ascontiguousarray(tile if channels == 3 else tile[:, :, 0]))


def pillow_file(tile, channels, exif=None, **options):
    buf = io.BytesIO()
    pillow_image(tile, channels).save(buf, "PNG", **({} if exif is None else {"exif": exif}), **options)
    return buf.getvalue()


def chunks(data):
    """[(type, payload)] of a PNG file; every chunk's CRC is checked on the way"""
    assert data[:8] == image_util.PNG_SIGNATURE
    out, at = [], 8
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload), kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data) and out[-1][0] == b"IEND"
    return out


def layout(parsed):
    """the chunk types in order, a file's consecutive IDATs as one (Pillow cuts its payload into IDATs of 64 KiB)"""
    kinds = [k for k, _ in parsed]
    return [k for i, k in enumerate(kinds) if not (k == b"IDAT" and i and kinds[i - 1] == b"IDAT")]


@functools.lru_cache(maxsize=None)
def _case(name, mode):
    """(emulator's file, channels, stats, Pillow's Z_RLE file of the same pixels in the same mode): computed once"""
    tile = _tile(name)
    stream, crc, ch, stats = emu_stream(tile, mode)
    got = image_util.png_file(tile.shape[1], tile.shape[0], ch, stream, crc)
    return got, ch, stats, pillow_file(tile, ch, compress_type=zlib.Z_RLE)


@pytest.mark.parametrize("name,mode", CASES)
def test_file_reopens_and_stream_is_the_stated_one(name, mode):
    tile = _tile(name)
    got, ch, _, want = _case(name, mode)
    assert ch == (3 if mode == "rgb" or not is_mono(tile) else 1)
    back = Image.open(io.BytesIO(got))
    assert back.mode == ("RGB" if ch == 3 else "L")
    assert np.array_equal(np.asarray(back), tile if ch == 3 else tile[:, :, 0])
    mine, theirs = chunks(got), chunks(want)
    assert [k for k, _ in mine] == layout(theirs) == [b"IHDR", b"IDAT", b"IEND"]
    assert [c for c in mine if c[0] != b"IDAT"] == [c for c in theirs if c[0] != b"IDAT"]
    payload = dict(mine)[b"IDAT"]
    assert payload[:2] == b"\x78\x9c"
    filtered, _ = png_oracle.filtered(tile, ch)
    assert zlib.decompress(payload) == filtered


@pytest.mark.parametrize("name", ["run_lengths", "runs_33x50", "runs_65x171", "zeros", "random_3x5", "mono_noise"])
def test_block_tokens_follow_the_run_rule(name):
    tile = _tile(name)
    for ch in (3, 1) if is_mono(tile) else (3,):
        stream, _ = png_oracle.filtered(tile, ch)
        for block in png_oracle.blocks(stream, tile.shape[1] * ch + 1):
            hist = np.zeros(286, np.uint32)
            src = np.frombuffer(block, np.uint8)
            _emu().emu_png_block_histogram(src.ctypes.data, src.size, hist.ctypes.data)
            assert np.array_equal(hist, png_oracle.histogram(block))


def test_the_set_reaches_the_corners():
    """conditions, not measurements: the run tile holds runs of exactly the lengths around a 258-match, a run through a row's end
    and one cut at a block's end; some block has no match (the no-distance-code form); the 15-bit limit binds on a golden tile"""
    tile = _tile("run_lengths")
    stream, types = png_oracle.filtered(tile, 1)
    assert not types.any()
    row = tile.shape[1] + 1
    first, second = png_oracle.blocks(stream, row)
    lengths = [n for v, n in png_oracle.runs(first) if v == 0] + [n for v, n in png_oracle.runs(second) if v == 0]
    for n in RUN_LENGTHS:
        assert n in lengths
    assert 7 + 1 + 5 in lengths  # row 10's tail, row 11's filter byte and head
    assert first.endswith(bytes(9)) and second.startswith(bytes(12)) and 9 in lengths and 12 in lengths  # cut at the block's end
    assert png_oracle.tokens(bytes(261)) == [("lit", 0), ("match", 258), ("lit", 0), ("lit", 0)]
    assert png_oracle.tokens(bytes(262)) == [("lit", 0), ("match", 258), ("match", 3)]
    assert png_oracle.tokens(bytes(3)) == [("lit", 0)] * 3 and png_oracle.tokens(bytes(4)) == [("lit", 0), ("match", 3)]
    assert _case("random_3x5", "rgb")[2][0] == 1  # its one block has no match
    assert any(_case(name, "rgb")[2][2] > 0 for name in SPECTROGRAM_TILES)
    assert max(_case(name, mode)[2][1] for name, mode in CASES) == 15


def test_file_with_spectrogram_exif():
    params = SpectrogramParams(stereo=True)
    exif_data = params.to_exif()
    exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(np.float32(12345678.0))
    exif = Image.Exif()
    exif.update(exif_data.items())
    colour = np.ascontiguousarray(_golden(STEREO_PNG)[100:164, 40:139])
    grey = np.ascontiguousarray(_golden(MONO_PNG)[100:164, 40:139])
    for tile, mode, ch in ((colour, "rgb", 3), (grey, "gray", 1), (grey, "auto", 1)):
        got = emu_file(tile, mode, exif)
        want = pillow_file(tile, ch, exif)  # Pillow's own save(f, "PNG", exif=e)
        mine, theirs = chunks(got), chunks(want)
        assert [k for k, _ in mine] == layout(theirs) == [b"IHDR", b"eXIf", b"IDAT", b"IEND"]
        assert [c for c in mine if c[0] != b"IDAT"] == [c for c in theirs if c[0] != b"IDAT"]
        back = Image.open(io.BytesIO(got))
        assert dict(back.getexif()) == dict(Image.open(io.BytesIO(want)).getexif()) == dict(exif)
        assert SpectrogramParams.from_exif(back.getexif()) == params
        assert back.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value] == 12345678.0
        assert np.array_equal(np.asarray(back), tile if ch == 3 else tile[:, :, 0])
        # bytes with the JPEG prefix are taken too
        assert image_util.png_file(tile.shape[1], tile.shape[0], ch, b"x", None, exif.tobytes())[:len(got) - len(dict(mine)[b"IDAT"]) - 24] == \
            got[:len(got) - len(dict(mine)[b"IDAT"]) - 24]


def test_gray_mode_flags_a_colour_tile():
    stream, crc, ch, _ = emu_stream(_tile("random_3x5"), "gray")
    assert (stream, crc, ch) == (b"", 0, 0)


# ---- the code builder alone ----------------------------------------------------------------------------------------------------
def _fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def _build(counts, limit):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    lens = np.full(counts.size, 99, np.uint8)
    codes = np.zeros(counts.size, np.uint16)
    used = _emu().emu_png_code_lengths(counts.ctypes.data, counts.size, limit, lens.ctypes.data, codes.ctypes.data)
    assert used == int((counts > 0).sum())
    return lens.astype(np.int64), codes


def _unlimited_depth(counts):
    """the longest code of Huffman's tree over the used symbols"""
    import heapq

    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def _padded(values, n):
    return np.asarray(list(values) + [0] * (n - len(values)), np.uint32)


BUILDER_CASES = {
    "fib44_of_286": (_padded(_fib(44), 286), 15, True),
    "fib40_then_ones_all_286": (np.asarray(_fib(40) + [1] * 246, np.uint32), 15, True),
    "fib44_scattered": (np.roll(_padded(_fib(44), 286), 173), 15, True),
    "fib19": (np.asarray(_fib(19), np.uint32), 7, True),
    "fib12_of_19": (_padded([0, 0, 0] + _fib(12), 19), 7, True),
    "one_symbol_and_eob": (np.bincount([7, 256], weights=[500, 1], minlength=286).astype(np.uint32), 15, False),
    "two_symbols": (np.bincount([0, 285], weights=[3, 3], minlength=286).astype(np.uint32), 15, False),
    "all_286_equal": (np.full(286, 9, np.uint32), 15, False),
    "all_286_ramp": (np.arange(1, 287, dtype=np.uint32), 15, False),
    "all_19_equal": (np.full(19, 2, np.uint32), 7, False),
    "two_of_19": (_padded([0, 5, 0, 0, 1], 19), 7, False),
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_code_builder(name):
    counts, limit, deep = BUILDER_CASES[name]
    assert (_unlimited_depth(counts) > limit) == deep
    lens, codes = _build(counts, limit)
    used = counts > 0
    assert (lens[used] >= 1).all() and (lens[~used] == 0).all() and lens.max() <= limit
    assert int((1 << (limit - lens[used])).sum()) == 1 << limit  # Kraft sum exactly 1
    # a more frequent symbol never has the longer code; among equal counts the lower symbol has the longer or equal one
    order = sorted(np.flatnonzero(used), key=lambda s: (counts[s], s))
    assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]))
    # the canonical code of RFC 1951 3.2.2, stored bit-reversed
    code, want = 0, {}
    for length in range(1, limit + 1):
        for s in np.flatnonzero(lens == length):
            want[int(s)] = int(format(code, f"0{length}b")[::-1], 2)
            code += 1
        code <<= 1
    assert {int(s): int(codes[s]) for s in np.flatnonzero(used)} == want
    if not deep:  # not limited: Huffman's own cost
        import heapq

        heap = [int(c) for c in counts if c]
        heapq.heapify(heap)
        cost = 0
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            cost += a + b
            heapq.heappush(heap, a + b)
        assert int((lens * counts.astype(np.int64)).sum()) == cost


def test_one_used_symbol_gets_a_companion():
    for s, other in ((0, 1), (5, 0)):
        lens, _ = _build(np.bincount([s], minlength=19).astype(np.uint32), 7)
        assert lens[s] == 1 and lens[other] == 1 and lens.sum() == 2


# ---- size ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPECTROGRAM_TILES)
def test_size_against_pillow_rle(name):
    for mode in modes_of(name):
        got, _, _, want = _case(name, mode)
        ratio = len(got) / len(want)
        print(f"{name} {mode}: {len(got)} bytes, Pillow Z_RLE {len(want)}, ratio {ratio:.4f}")
        assert ratio <= RATIO_BOUND, (name, mode, len(got), len(want))


def test_capacity_holds_and_is_the_stated_formula():
    lib, load = _emu(), _hip.load_library()
    for name, mode in CASES:  # (emu_stream asserts it for every case; uniform random bytes in RGB among them)
        tile = _tile(name)
        got, ch, _, _ = _case(name, mode)
        assert len(dict(chunks(got))[b"IDAT"]) <= lib.emu_png_stream_capacity(tile.shape[0], tile.shape[1], ch)
    for H, W, ch in [(512, 512, 3), (512, 512, 1), (1, 1, 3), (33, 50, 1), (65535, 5, 3)]:
        S, B = H * (W * ch + 1), -(-H // 32)
        want = 2 + (B * 4107 + 15 * S + 7) // 8 + 4
        assert load.rfx_png_stream_capacity(H, W, ch) == want == lib.emu_png_stream_capacity(H, W, ch)
    # a tile of uniform random bytes at 512 x 512 stays inside it with room to spare: 8 bits a byte and the headers, of 15
    stream, _, _, _ = emu_stream(np.random.default_rng(3).integers(0, 256, size=(512, 512, 3), dtype=np.uint8), "rgb")
    assert 512 * 1537 < len(stream) < load.rfx_png_stream_capacity(512, 512, 3) * 0.6


def test_queries_and_refusals():
    lib = _hip.load_library()
    assert lib.rfx_png_stream_capacity(512, 65536, 3) == 0 and lib.rfx_png_stream_capacity(0, 8, 3) == 0
    assert lib.rfx_png_stream_capacity(8, 8, 2) == 0 and lib.rfx_png_stream_capacity(8, 8, 4) == 0
    assert lib.rfx_png_encode_workspace_bytes(1, 512, 65536) == 0 and lib.rfx_png_encode_workspace_bytes(0, 8, 8) == 0
    assert lib.rfx_png_encode_workspace_bytes(1, 40000, 40000) == 0  # its capacity is past int32
    assert lib.rfx_png_encode_workspace_bytes(3, 512, 501) > 3 * (512 * 1504 + lib.rfx_png_stream_capacity(512, 501, 3))
    # refused before anything is launched (no GPU here, no buffers)
    call = lambda N, H, W, mode: lib.rfx_png_encode_u8(None, N, H, W, mode, None, None, None, None, None, None)  # noqa: E731
    assert call(1, 8, 65536, 0) == -4 and b"65535" in lib.rfx_last_error()  # RFX_ERR_UNSUPPORTED
    assert call(1, 40000, 40000, 0) == -4 and b"int32" in lib.rfx_last_error()
    assert call(40000, 65535, 1, 0) == -4 and b"one launch" in lib.rfx_last_error()
    assert call(0, 8, 8, 0) == -1 and call(1, 8, 8, 3) == -1 and b"mode" in lib.rfx_last_error()  # RFX_ERR_INVALID
    assert call(1, 8, 8, 0) == -1 and b"null" in lib.rfx_last_error()


def test_header_arguments():
    with pytest.raises(ValueError):
        image_util.png_file(65536, 8, 3, b"")
    with pytest.raises(ValueError):
        image_util.png_file(8, 0, 3, b"")
    with pytest.raises(ValueError):
        image_util.png_file(8, 8, 2, b"")
    tile = np.zeros((8, 8, 3), np.uint8)
    want = pillow_file(tile, 3)
    assert image_util.png_file(8, 8, 3, dict(chunks(want))[b"IDAT"]) == want  # the layout Pillow writes, CRC computed on the host
    assert image_util.png_exif_bytes(None) == b"" and image_util.png_exif_bytes(b"Exif\0\0II*\0") == b"II*\0"


def test_cli_flags():
    """--png-writer / --png-mode parse on both commands, default to Pillow's route, and --png-mode without the device writer is an
    error of the command line (the device route itself: tests/test_gpu_png.py)"""
    from riffusion import cli

    parser = cli.build_parser()
    one = vars(parser.parse_args(["audio-to-image", "--audio", "a.wav", "--image", "b.png"]))
    assert (one["png_writer"], one["png_mode"]) == ("pillow", "rgb")
    many = vars(parser.parse_args(["audio-to-images-batch", "--audio-dir", "a", "--output-dir", "b", "--png-writer", "device", "--png-mode", "auto"]))
    assert (many["png_writer"], many["png_mode"]) == ("device", "auto")
    for bad in (["--png-mode", "gray"], ["--png-writer", "zlib"], ["--png-writer", "device", "--png-mode", "grey"]):
        with pytest.raises(SystemExit):
            cli.main(["audio-to-image", "--audio", "a.wav", "--image", "b.png"] + bad)
        with pytest.raises(SystemExit):
            cli.main(["audio-to-images-batch", "--audio-dir", "a", "--output-dir", "b"] + bad)
    with pytest.raises(ValueError, match="png-writer device"):
        cli.audio_to_images_batch(audio_dir="a", output_dir="b", png_mode="auto")
