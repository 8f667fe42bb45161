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
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_oracle
from png_cases import (BUILDER_CASES, CASES, MONO_PNG, RATIO_BOUND, RUN_LENGTHS, SPECTROGRAM_TILES, STEREO_PNG, _build, _case, _emu, _golden, _tile,
                       _unlimited_depth, chunks, emu_file, emu_stream, is_mono, layout, modes_of, pillow_file)
from riffusion import _hip
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import image_util


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
