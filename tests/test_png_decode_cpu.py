"""
CPU checks of the PNG decoder (csrc/rfx_png_dec_core.h, compiled for the host with tests/emu/rfx_png_dec_emu.cpp, in the kernels'
two stages) and of image_util.png_parse: the emulator's pixels against `np.asarray(Image.open(f).convert("RGB"))` of the Pillow on
this machine and its filtered bytes against `zlib.decompress`, byte for byte, no tolerance.  The files (tests/png_decode_cases.py):
the ten golden PNGs; Pillow's saves of small tiles in modes L, RGB, RGBA and P with stored, fixed and dynamic blocks; the device
writer's own files; hand-built deflate streams (tests/deflate_writer.py); hand-written filter rows; damaged streams, each with the
status it must get.  A stand-alone build of the emulator under AddressSanitizer and UBSan runs the same inputs and must give the
same statuses and pixels as the plain build.  Nothing sanitized is loaded into Python.
"""
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import deflate_writer as dw
import emu_build
import png_decode_cases as C
from png_cases import emu_file
from riffusion.util import image_util


def decode_one(data):
    info, stream = C.parts_of(data)
    rgb, status = C.emu_decode([stream], info.height, info.width, info.color_type, info.palette[None], [info.palette_entries])
    return int(status[0]), rgb[0]


# ---- golden files -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,data", C.golden_files(), ids=[n for n, _ in C.golden_files()])
def test_golden_pixels_and_exif_equal_pillow(name, data):
    status, got = decode_one(data)
    assert status == 0
    assert np.array_equal(got, C.pillow_pixels(data))
    exif = Image.Exif()
    info = image_util.png_parse(data)
    if info.exif:
        exif.load(info.exif)
    assert dict(exif) == dict(Image.open(io.BytesIO(data)).getexif())


def test_there_are_ten_goldens_and_their_kinds():
    infos = [image_util.png_parse(d) for _, d in C.golden_files()]
    assert len(infos) == 10 and all(i.ok_for_device for i in infos)
    assert {i.color_type for i in infos} == {0, 2, 3}
    assert sorted(len(i.idat) for i in infos)[-2:] == [5, 6]


# ---- Pillow's saves -----------------------------------------------------------------------------------------------------------------------
def test_pillow_saves_equal_pillow():
    files = C.pillow_saves()
    got = C.decode_files(C.emu_decode, files)
    for name, data in files:
        status, pixels = got[name]
        assert status == 0, name
        assert np.array_equal(pixels, C.pillow_pixels(data)), name


def block_types(stream):
    """the types of a stream's first block (enough to tell what a save option made)"""
    return (stream[2] >> 1) & 3


def test_the_saves_reach_every_block_kind_and_mode():
    files = dict(C.pillow_saves())
    infos = {n: image_util.png_parse(d) for n, d in files.items()}
    assert {i.color_type for i in infos.values()} == {0, 2, 3, 6}
    assert all(i.palette_entries > 16 for i in infos.values() if i.color_type == 3)
    first = {n: block_types(C.parts_of(d)[1]) for n, d in files.items()}
    assert all(first[n] == 0 for n in files if n.endswith("_stored"))
    assert all(first[n] == 1 for n in files if n.endswith("_fixed"))
    assert any(first[n] == 2 for n in files if n.endswith("_default")) and any(first[n] == 2 for n in files if n.endswith("_optimize"))
    for option in C.SAVE_OPTIONS:
        assert {infos[n].color_type for n in files if n.endswith("_" + option)} == {0, 2, 3, 6}, option
    # several stored blocks; rows of more than one piece
    info, stream = C.parts_of(files["random_90x250_RGB_stored"])
    assert len(zlib.decompress(stream)) > 65535
    assert infos["golden_2x3100_RGBA_default"].width * 4 > C.emu().emu_png_dec_seg_bytes() < infos["random_3x12289_L_default"].width


def test_device_writer_files():
    for make, h, w in ((C._golden_crop, 70, 87), (C._random, 33, 50)):
        tile = make(h, w)
        grey = np.repeat(tile[:, :, :1], 3, axis=2)
        for t, mode in ((tile, "rgb"), (grey, "gray"), (grey, "auto"), (tile, "auto")):
            data = emu_file(t, mode)
            status, got = decode_one(data)
            assert status == 0 and np.array_equal(got, t) and np.array_equal(got, C.pillow_pixels(data)), (h, w, mode)


# ---- hand-built streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in C.hand_built()])
def test_hand_built_streams(name):
    data = dict(C.hand_built())[name]
    info, stream = C.parts_of(data)
    raw = zlib.decompress(stream)  # zlib takes the stream, and gives what the test meant
    assert len(raw) == info.width + 1
    status, got = decode_one(data)
    assert status == 0
    assert np.array_equal(got, C.pillow_pixels(data))
    assert got[0, :, 0].tobytes() == raw[1:]


def test_deflate_writer_symbols():
    lengths = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    for n in range(3, 259):
        s, e, v = dw.length_symbol(n)
        assert lengths[s - 257] + v == n and v < (1 << e) and (s == 285 or n < lengths[s - 256])
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 24576, 24577, 32767, 32768):
        s, e, v = dw.distance_symbol(d)
        base = d - v
        assert 0 <= s < 30 and v < (1 << e) and base == (s + 1 if s < 4 else ((2 + (s & 1)) << ((s >> 1) - 1)) + 1)


# ---- filters ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in C.filter_files()])
def test_filters(name):
    data = dict(C.filter_files())[name]
    status, got = decode_one(data)
    assert status == 0
    assert np.array_equal(got, C.pillow_pixels(data))


def test_paeth_ties_and_odd_average_are_in_the_file():
    data = dict(C.filter_files())["paeth_ties_and_odd_average"]
    px = C.pillow_pixels(data)[:, :, 0].astype(int)
    kinds = set()
    for x in range(px.shape[1]):
        a, b, c = (px[1, x - 1], px[0, x], px[0, x - 1]) if x else (0, px[0, 0], 0)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        kinds |= {k for k, hit in (("all", pa == pb == pc), ("left_up", pa == pb < pc), ("up_upleft", pb == pc < pa), ("left_upleft", pa == pc < pb)) if hit}
    assert kinds >= {"all", "left_up", "up_upleft", "left_upleft"}
    assert (0 + px[1, 0]) % 2 == 1 and px[2, 0] == (1 + px[1, 0] // 2) % 256


# ---- damaged streams ---------------------------------------------------------------------------------------------------------------------
def test_damaged_streams_get_their_status_and_leave_the_others_alone():
    cases = C.damaged()
    good = cases[0][1]
    streams = [good] + [s for _, s, _ in cases] + [good]
    rgb, status = C.emu_decode(streams, C.DAMAGE_H, C.DAMAGE_W, 2)
    want = C.pillow_pixels(C.damaged_file(good))
    assert status[0] == 0 and status[-1] == 0 and np.array_equal(rgb[0], want) and np.array_equal(rgb[-1], want)
    for (name, _, expected), got in zip(cases, status[1:-1]):
        assert got == expected, (name, got, expected)
    assert {e for _, _, e in cases} == set(range(12)) - {0, 12} | {0}  # every inflate status and the filter's; 12 below
    _, stream, pal, entries = C.palette_damage()
    rgb, status = C.emu_decode([stream], 2, 3, 3, pal[None], [entries])
    assert status[0] == 12
    rgb, status = C.emu_decode([stream], 2, 3, 3, pal[None], [entries + 1])
    assert status[0] == 0


class EmuPlan:
    """Plan.png_decode by the emulator, for images_from_png_bytes without a GPU"""
    device = "cpu"

    def png_decode(self, streams, H, W, color_type, palettes=None, entries=None):
        import torch

        rgb, status = C.emu_decode(streams, H, W, color_type, palettes, entries)
        return torch.from_numpy(rgb), status


def host_route(data):
    """(pixels, exif dict) as the host route gives them, or the exception's type"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            return image_util.rgb_array_from_image(im), dict(im.getexif())
    except Exception as e:  # noqa: BLE001 - whatever Pillow raises is what the entry must raise
        return type(e)


def converter_with_emulator(monkeypatch):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramImageConverter(params=SpectrogramParams(), device="cuda")
    monkeypatch.setattr(conv.converter, "_plan", lambda: EmuPlan())
    return conv


def test_images_from_png_bytes_returns_what_pillow_returns_or_raises(monkeypatch):
    conv = converter_with_emulator(monkeypatch)
    files = [C.damaged_file(s) for name, s, _ in C.damaged() if not name.startswith("truncated_at_") or name.endswith(("_0", "_7", "_20"))]
    files.append(C.palette_damage()[0])
    for data in files:
        want = host_route(data)
        if isinstance(want, type):
            with pytest.raises(want):
                conv.images_from_png_bytes([data])
        else:
            tiles, exifs = conv.images_from_png_bytes([data])
            assert np.array_equal(tiles[0], want[0]) and dict(exifs[0]) == want[1]


def test_images_from_png_bytes_mixed_list(monkeypatch):
    conv = converter_with_emulator(monkeypatch)
    golden = dict(C.golden_files())
    rgb16, interlaced, jpeg = C.host_only_files()
    assert not any(image_util.png_parse(f).ok_for_device for f in (rgb16, interlaced, jpeg))
    files = [golden["og_beat_64.png"], C.pillow_saves()[5][1], rgb16, interlaced, jpeg, C.damaged_file(dict((n, s) for n, s, _ in C.damaged())["left_over_byte"]),
             golden["og_beat_64.png"]]
    tiles, exifs = conv.images_from_png_bytes(files, tiles_per_call=1)
    assert isinstance(tiles, list) and len(tiles) == len(files)
    for data, tile, exif in zip(files, tiles, exifs):
        want = host_route(data)
        assert np.array_equal(tile, want[0]) and dict(exif) == want[1]
    batch, _ = conv.images_from_png_bytes([golden["og_beat_64.png"]] * 3)
    assert batch.shape == (3, 512, 64, 3)
    with pytest.raises(ValueError):
        conv.images_from_png_bytes(files, tiles_per_call=0)


def test_random_corruptions_never_give_other_pixels():
    """2000 seeded single-byte corruptions of a 33 x 50 tile's stream: a status, or Pillow's pixels of the corrupted file"""
    tile = C._golden_crop(33, 50)
    data = C.pillow_png(Image.fromarray(tile))
    info, stream = C.parts_of(data)
    rng = np.random.default_rng(2024)
    streams = []
    for _ in range(2000):
        s = bytearray(stream)
        at = int(rng.integers(0, len(s)))
        s[at] ^= int(rng.integers(1, 256))
        streams.append(bytes(s))
    rgb, status = C.emu_decode(streams, 33, 50, 2)
    accepted = np.flatnonzero(status == 0)
    print("corruptions accepted:", len(accepted), "statuses:", np.bincount(status, minlength=13))
    for i in accepted:
        want = host_route(image_util.png_file(50, 33, 3, streams[i]))
        assert not isinstance(want, type) and np.array_equal(rgb[i], want[0]), i
    assert (status != 0).sum() > 1000  # the corruptions do damage


# ---- the sanitizer build ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    flags = ("-std=c++17", "-DRFX_PNGD_EMU_MAIN")
    return (tmp_path_factory.mktemp("png_dec_programs"), emu_build.program(C.EMU_SRC, "-O1", "-g", *flags),
            emu_build.sanitized_program(C.EMU_SRC, *flags, static=False))


def run_program(program, directory, name, case):
    src, out = str(directory / (name + ".case")), str(directory / (name + "." + os.path.basename(program)))
    with open(src, "wb") as f:
        f.write(case)
    done = subprocess.run([program, src, out], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "batch 0", (name, done.returncode, done.stdout, done.stderr[-2000:])
    with open(out, "rb") as f:
        return f.read()


def test_sanitized_program_equals_the_plain_one(programs):
    d, plain, sanitized = programs
    cases = []
    groups = {}
    for name, data in C.golden_files() + C.hand_built() + C.filter_files():
        info, stream = C.parts_of(data)
        groups.setdefault((info.height, info.width, info.color_type), []).append((info, stream))
    for k, ((H, W, ct), members) in enumerate(groups.items()):
        cases.append((f"group{k}", len(members), H, W, C.case_file_bytes([m[1] for m in members], H, W, ct, np.stack([m[0].palette for m in members]),
                                                                        [m[0].palette_entries for m in members]), None))
    damaged = C.damaged()
    cases.append(("damaged", len(damaged), C.DAMAGE_H, C.DAMAGE_W, C.case_file_bytes([s for _, s, _ in damaged], C.DAMAGE_H, C.DAMAGE_W, 2),
                  [e for _, _, e in damaged]))
    _, stream, pal, entries = C.palette_damage()
    cases.append(("palette", 1, 2, 3, C.case_file_bytes([stream], 2, 3, 3, pal[None], [entries]), [12]))
    for name, n, H, W, case, expected in cases:
        a = run_program(plain, d, name, case)
        b = run_program(sanitized, d, name, case)
        assert a == b, name
        status = np.frombuffer(a[:4 * n], np.int32)
        assert len(a) == 4 * n + n * H * W * 3
        if expected is None:
            assert not status.any(), name
        else:
            assert list(status) == expected, name


# ---- png_parse ------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, payload=b"", crc=None):
    return image_util._png_chunk(kind, payload, crc)


def ihdr(w=4, h=3, depth=8, ct=2, comp=0, filt=0, lace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, comp, filt, lace))


def png(*chunks):
    return image_util.PNG_SIGNATURE + b"".join(chunks)


GOOD_IDAT = zlib.compress(bytes(3 * 13))
END = chunk(b"IEND")


def test_png_parse_reasons():
    parse = image_util.png_parse
    ok = parse(png(ihdr(), chunk(b"IDAT", GOOD_IDAT), END))
    assert ok.ok_for_device and ok.reason == "" and (ok.width, ok.height, ok.color_type, ok.channels) == (4, 3, 2, 3)
    assert [parse(png(ihdr(ct=t), chunk(b"PLTE", bytes(6)), chunk(b"IDAT", GOOD_IDAT), END)).channels for t in (0, 2, 3, 6)] == [1, 3, 1, 4]
    reasons = {
        "bit depth 16": png(ihdr(depth=16), chunk(b"IDAT", GOOD_IDAT), END),
        "bit depth 4": png(ihdr(depth=4, ct=0), chunk(b"IDAT", GOOD_IDAT), END),
        "colour type 4": png(ihdr(ct=4), chunk(b"IDAT", GOOD_IDAT), END),
        "Adam7": png(ihdr(lace=1), chunk(b"IDAT", GOOD_IDAT), END),
        "APNG": png(ihdr(), chunk(b"acTL", bytes(8)), chunk(b"IDAT", GOOD_IDAT), END),
        "unknown critical chunk": png(ihdr(), chunk(b"ABCD", b"x"), chunk(b"IDAT", GOOD_IDAT), END),
        "EXIF in a text chunk": png(ihdr(), chunk(b"tEXt", b"Raw profile type exif\x00abc"), chunk(b"IDAT", GOOD_IDAT), END),
        "truncated": png(ihdr(), chunk(b"IDAT", GOOD_IDAT)),
        "not a PNG": b"\xff\xd8\xff\xe0" + bytes(20),
        "CRC mismatch": png(ihdr(), chunk(b"IDAT", GOOD_IDAT, crc=1), END),
        "not consecutive": png(ihdr(), chunk(b"IDAT", GOOD_IDAT[:5]), chunk(b"gAMA", bytes(4)), chunk(b"IDAT", GOOD_IDAT[5:]), END),
        "no IDAT": png(ihdr(), END),
        "without PLTE": png(ihdr(ct=3), chunk(b"IDAT", GOOD_IDAT), END),
        "PLTE": png(ihdr(ct=3), chunk(b"PLTE", bytes(7)), chunk(b"IDAT", GOOD_IDAT), END),
        "IHDR is not the first": png(chunk(b"gAMA", bytes(4)), ihdr(), chunk(b"IDAT", GOOD_IDAT), END),
        "compression or filter method": png(ihdr(comp=1), chunk(b"IDAT", GOOD_IDAT), END),
    }
    for word, data in reasons.items():
        info = parse(data)
        assert not info.ok_for_device and word in info.reason, (word, info.reason)
    for kind in (b"fcTL", b"fdAT", b"zTXt", b"iTXt"):
        payload = b"Raw profile type exif\x00abc" if kind[1:] != b"cTL" and kind != b"fdAT" else bytes(8)
        assert not parse(png(ihdr(), chunk(kind, payload), chunk(b"IDAT", GOOD_IDAT), END)).ok_for_device, kind


def test_png_parse_details():
    parse = image_util.png_parse
    exif = b"MM\x00\x2a\x00\x00\x00\x08\x00\x00"
    # eXIf after IDAT; skipped ancillary chunks; the text key beside a real eXIf does not matter
    info = parse(png(ihdr(), chunk(b"gAMA", bytes(4)), chunk(b"tEXt", b"Raw profile type exif\x00abc"), chunk(b"tRNS", bytes(6)),
                     chunk(b"IDAT", GOOD_IDAT), chunk(b"eXIf", exif), chunk(b"tEXt", b"Comment\x00hello"), END))
    assert info.ok_for_device and info.exif == exif
    # a CRC error in an ancillary chunk keeps the file on the host
    bad = parse(png(ihdr(), chunk(b"gAMA", bytes(4), crc=7), chunk(b"IDAT", GOOD_IDAT), END))
    assert not bad.ok_for_device and "CRC" in bad.reason
    # split IDATs with an empty one among them: the ranges in file order, their concatenation the stream
    data = png(ihdr(), chunk(b"IDAT", GOOD_IDAT[:3]), chunk(b"IDAT"), chunk(b"IDAT", GOOD_IDAT[3:]), END)
    info = parse(data)
    assert info.ok_for_device and len(info.idat) == 3 and b"".join(data[a:b] for a, b in info.idat) == GOOD_IDAT
    status, got = decode_one(data)
    assert status == 0 and not got.any()
    # the palette: entries and zeros behind them
    info = parse(png(ihdr(ct=3), chunk(b"PLTE", bytes(range(1, 10))), chunk(b"IDAT", GOOD_IDAT), END))
    assert info.palette_entries == 3 and info.palette.shape == (256, 3) and info.palette[:3].reshape(-1).tolist() == list(range(1, 10)) and not info.palette[3:].any()
    # never raises: every prefix of a good file, and none of them is taken
    good = dict(C.golden_files())["og_beat_64.png"]
    for n in list(range(0, 200)) + list(range(len(good) - 40, len(good))):
        assert not parse(good[:n]).ok_for_device
    assert parse(good).ok_for_device
    for junk in (b"", b"\x89PNG", bytes(100), image_util.PNG_SIGNATURE + b"\xff" * 40):
        assert not parse(junk).ok_for_device


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_cli_png_reader_flag(tmp_path, monkeypatch):
    from riffusion import cli

    parser = cli.build_parser()
    for command, extra in (("images-to-audio-batch", ["--image-dir", "a", "--output-dir", "b"]), ("image-to-audio", ["--image", "a", "--audio", "b"])):
        assert vars(parser.parse_args([command] + extra))["png_reader"] == "pillow"
        assert vars(parser.parse_args([command] + extra + ["--png-reader", "device"]))["png_reader"] == "device"
        with pytest.raises(SystemExit):
            parser.parse_args([command] + extra + ["--png-reader", "gpu"])
    with pytest.raises(ValueError):
        cli.images_to_audio_batch(image_dir="a", output_dir=str(tmp_path / "o"), png_reader="gpu")
    # the default leaves _load_tiles on Pillow: no converter entry is touched
    golden = os.path.join(C.GOLDEN, "og_beat_64.png")
    tiles = cli._load_tiles(None, [golden, golden], "png")
    assert tiles.shape == (2, 512, 64, 3) and np.array_equal(tiles[0], C.pillow_pixels(open(golden, "rb").read()))

    class Recorder:
        def images_from_png_bytes(self, files, return_device=False):
            self.seen = (len(files), return_device)
            return "tiles", []

    rec = Recorder()
    assert cli._load_tiles(rec, [golden], "png", "device") == "tiles" and rec.seen == (1, True)
    groups_pillow = cli._tile_groups([golden], "png")
    groups_device = cli._tile_groups([golden], "png", "device")
    assert groups_pillow == groups_device
