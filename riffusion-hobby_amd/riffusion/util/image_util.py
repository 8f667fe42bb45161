"""
uint8 spectrogram image <-> float mel amplitudes.

Same functions and semantics as the reference's `riffusion/util/image_util.py:13-122`.  The power
curve has only finitely many cases on either side (256 pixel values when decoding, 256 output
levels when encoding), so it is tabulated with numpy's own float32 arithmetic:

* `decode_lut`       - the 256 float32 values numpy's chain `255-p, /255, **(1/power), *max_value`
                       produces (image_util.py:96-108);
* `encode_thresholds`- for each level v the smallest float32 ratio x/max that numpy's chain
                       `**power, *255, 255-, astype(uint8)` maps to a value <= v (image_util.py:32-41).

The HIP kernels (csrc/rfx_codec.hip) consume exactly these tables, which makes the device codec
bit-exact to the reference given the same float input; the numpy functions below use the same
tables so host and device agree byte for byte.
"""
import functools
import re
import struct
import typing as T
import zlib

import numpy as np
from PIL import Image

from riffusion.spectrogram_params import SpectrogramParams


@functools.lru_cache(maxsize=32)
def decode_lut(power: float = 0.25, max_value: float = 30e6) -> np.ndarray:
    p = np.arange(256, dtype=np.uint8).astype(np.float32)
    p = 255 - p
    p = p / 255
    p = np.power(p, 1 / power)
    p = p * max_value
    return np.ascontiguousarray(p, dtype=np.float32)


@functools.lru_cache(maxsize=1)
def pipeline_input_lut() -> np.ndarray:
    """The value riffusion_pipeline.py:447-452 (preprocess_image) gives each pixel byte: numpy's float32 `/ 255.0`, then torch's
    float32 `2.0 * x - 1.0` - the reference's own operations, on the 256 possible bytes."""
    import torch

    p = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    return (2.0 * torch.from_numpy(p) - 1.0).numpy()


def _quantise_ratio(ratio: np.ndarray, power: float) -> np.ndarray:
    """numpy's own chain from image_util.py:32-41 applied to float32 ratios x/max."""
    d = np.power(ratio, power)
    d = d * 255
    d = 255 - d
    return d.astype(np.uint8)


@functools.lru_cache(maxsize=32)
def encode_thresholds(power: float = 0.25) -> np.ndarray:
    """thr[v], v = 0..254: smallest float32 r in [0, 1] with quantise(r) <= v (non-increasing in v)."""
    one = np.array([1.0], dtype=np.float32).view(np.uint32)[0]
    levels = np.arange(255, dtype=np.int64)
    lo = np.zeros(255, dtype=np.int64)  # invariant: quantise(lo-1) > v  (or lo == 0)
    hi = np.full(255, int(one), dtype=np.int64)  # invariant: quantise(hi) <= v  (quantise(1.0) == 0)
    while np.any(lo < hi):
        mid = (lo + hi) // 2
        q = _quantise_ratio(mid.astype(np.uint32).view(np.float32), power).astype(np.int64)
        ok = q <= levels
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid + 1)
    return np.ascontiguousarray(lo.astype(np.uint32).view(np.float32))


def quantise_spectrogram(spectrogram: np.ndarray, power: float = 0.25) -> np.ndarray:
    """(C, M, T) float32 -> (C, M, T) uint8: image_util.py:27-41 through the threshold table."""
    spectrogram = np.asarray(spectrogram, dtype=np.float32)
    ratio = spectrogram / np.max(spectrogram)
    thr = encode_thresholds(float(power))
    # q = number of thresholds strictly above the ratio; thr is non-increasing, search its reverse
    asc = thr[::-1]
    q = len(thr) - np.searchsorted(asc, ratio, side="right")
    return q.astype(np.uint8)


def image_from_spectrogram(spectrogram: np.ndarray, power: float = 0.25) -> Image.Image:
    """
    (channels, frequency, time) magnitudes -> RGB image (frequency, time), low frequencies at the
    bottom.  Mono is replicated into R=G=B, stereo goes to (0, left, right) - image_util.py:44-54.
    """
    data = quantise_spectrogram(spectrogram, power)
    if data.shape[0] == 1:
        rgb = np.repeat(data[0][:, :, None], 3, axis=2)
    elif data.shape[0] == 2:
        rgb = np.stack([np.zeros_like(data[0]), data[0], data[1]], axis=2)
    else:
        raise NotImplementedError(f"Unsupported number of channels: {data.shape[0]}")
    return Image.fromarray(np.ascontiguousarray(rgb[::-1]), mode="RGB")


def rgb_array_from_image(image: Image.Image) -> np.ndarray:
    """PIL image of any of the modes the reference accepts -> (H, W, 3) uint8 (image_util.py:81-82)."""
    if image.mode in ("P", "L"):
        image = image.convert("RGB")
    arr = np.array(image)
    if arr.ndim != 3 or arr.shape[2] < 3:
        raise ValueError(f"unsupported image mode {image.mode}")
    return np.ascontiguousarray(arr[:, :, :3])


def spectrogram_from_image(
    image: Image.Image,
    power: float = 0.25,
    stereo: bool = False,
    max_value: float = 30e6,
) -> np.ndarray:
    """RGB image -> (channels, frequency, time) float32 magnitudes (inverse of the above up to quantisation)."""
    rgb = rgb_array_from_image(image)[::-1]
    planes = rgb[:, :, [1, 2]] if stereo else rgb[:, :, 0:1]
    lut = decode_lut(float(power), float(max_value))
    return np.ascontiguousarray(lut[planes.transpose(2, 0, 1)])


def hold_mask_from_image(mask_image: Image.Image, keep_threshold: float = 0.5) -> np.ndarray:
    """A partial regeneration's mask image -> (n_mels, T) bool, True where the source is kept, in spectrogram orientation (band 0
    first: Y flipped, as `spectrogram_from_image` does).  The reference's convention (riffusion_pipeline.py:455-477): white is
    repainted, black is kept, and the latents are blended with 1 - mask; a pixel is held where 1 - L / 255 >= keep_threshold, L its
    luminance (`convert("L")`).  No resizing: the caller brings the mask to the tile's size."""
    if not (0.0 <= float(keep_threshold) <= 1.0):
        raise ValueError(f"keep_threshold must be in [0, 1], got {keep_threshold}")
    lum = np.asarray(mask_image.convert("L"), dtype=np.float64)[::-1]
    return np.ascontiguousarray(1.0 - lum / 255.0 >= float(keep_threshold))


def exif_from_image(pil_image: Image.Image) -> T.Dict[str, T.Any]:
    """EXIF of a spectrogram image as {tag name: value} (image_util.py:113-122)."""
    exif = pil_image.getexif()
    if exif is None or len(exif) == 0:
        return {}
    return {SpectrogramParams.ExifTags(key).name: val for key, val in exif.items()}


# ---- JPEG: everything of a file that does not depend on the pixels (the device writes the scan: rfx_jpeg_encode_u8) ----------
# ITU T.81 Annex K.3, the tables libjpeg (and so Pillow, without `optimize`) puts into DHT: (class << 4 | id, BITS, HUFFVAL)
JPEG_HUFFMAN_TABLES: T.Tuple[T.Tuple[int, bytes, bytes], ...] = (
    (0x00, bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x10, bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x11, bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)
# zigzag position -> natural (row-major) index: DQT carries a table in zigzag order
JPEG_NATURAL_ORDER = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                      47, 55, 62, 63)
JPEG_MAX_SIZE = 65535


def _jpeg_segment(marker: int, payload: bytes) -> bytes:
    if len(payload) + 2 > 65535:
        raise ValueError(f"JPEG segment FF{marker:02X} of {len(payload)} bytes is longer than a marker segment holds")
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_exif_bytes(exif: T.Any) -> bytes:
    """What Pillow's JPEG writer makes of its `exif` argument: an `Image.Exif` as `tobytes()`, bytes as they are, None as none."""
    if exif is None:
        return b""
    return exif.tobytes() if isinstance(exif, Image.Exif) else bytes(exif)


def jpeg_header_parts(width: int, height: int, quality: int = 75, qtables: T.Optional[np.ndarray] = None) -> T.Tuple[bytes, bytes]:
    """`jpeg_header` without the EXIF: (what comes before APP1, what comes after it) - the same for every tile of a batch."""
    width, height = int(width), int(height)
    if not (1 <= width <= JPEG_MAX_SIZE and 1 <= height <= JPEG_MAX_SIZE):
        raise ValueError(f"a JPEG holds 1 .. {JPEG_MAX_SIZE} rows and columns, got {width} x {height}")
    if qtables is None:
        from riffusion import _hip

        qtables = _hip.jpeg_quant_tables(quality)
    qtables = np.asarray(qtables)
    if qtables.shape != (2, 64) or qtables.min() < 1 or qtables.max() > 255:
        raise ValueError("qtables must be (2, 64) with entries in 1 .. 255")
    head = b"\xff\xd8" + _jpeg_segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out = [_jpeg_segment(0xDB, bytes([i]) + bytes(int(qtables[i][n]) for n in JPEG_NATURAL_ORDER)) for i in range(2)]
    # 8 bits, three components: Y 2 x 2 with table 0, Cb and Cr 1 x 1 with table 1
    out.append(_jpeg_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, bits, vals in JPEG_HUFFMAN_TABLES:
        out.append(_jpeg_segment(0xC4, bytes([tc_th]) + bits + vals))
    out.append(_jpeg_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return head, b"".join(out)


def jpeg_header(width: int, height: int, quality: int = 75, exif_bytes: bytes = b"", qtables: T.Optional[np.ndarray] = None) -> bytes:
    """
    The bytes of `Image.save(f, "JPEG", quality=quality, exif=...)` of an RGB image up to the scan: SOI, APP0 (JFIF 1.01, no
    units, density 1:1), APP1 with `exif_bytes` (`Image.Exif.tobytes()`, which starts with b"Exif\\0\\0"; empty: no APP1), the two
    quantisation tables, SOF0 (4:2:0), the four Huffman tables, SOS.  `qtables`: the (2, 64) tables in natural order; by
    default those of `quality` from the library (rfx_jpeg_quant_tables, host only).
    """
    head, tail = jpeg_header_parts(width, height, quality, qtables)
    return head + (_jpeg_segment(0xE1, bytes(exif_bytes)) if exif_bytes else b"") + tail


# ---- PNG: everything of a file but the IDAT payload (the device writes that and its CRC: rfx_png_encode_u8) --------------------
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_MAX_SIZE = 65535  # what rfx_png_encode_u8 takes per axis


def _png_chunk(kind: bytes, payload: bytes, crc: T.Optional[int] = None) -> bytes:
    if len(payload) >= 1 << 31:
        raise ValueError(f"PNG chunk {kind!r} of {len(payload)} bytes is longer than a chunk holds")
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) if crc is None else int(crc) & 0xFFFFFFFF)


def png_exif_bytes(exif: T.Any) -> bytes:
    """What Pillow's PNG writer puts into eXIf for its `exif` argument: an `Image.Exif` as `tobytes()`, bytes as they are, either
    without the b"Exif\\0\\0" prefix; None as none."""
    data = jpeg_exif_bytes(exif)
    return data[6:] if data.startswith(b"Exif\x00\x00") else data


def png_file(width: int, height: int, channels: int, idat_stream: bytes, idat_crc: T.Optional[int] = None, exif_bytes: bytes = b"") -> bytes:
    """
    A PNG file around one IDAT payload, in the layout of Pillow's `Image.save(f, "PNG", exif=...)`: signature, IHDR (bit depth 8,
    colour type 2 for `channels` 3 and 0 for 1, no interlace), eXIf with `exif_bytes` (a b"Exif\\0\\0" prefix is dropped; empty:
    no chunk), one IDAT with `idat_stream` (a zlib stream of the filtered rows: rfx_png_encode_u8) and IEND.  `idat_crc`: the
    CRC-32 of b"IDAT" + idat_stream when the caller has it (the device computes it); None: computed here.
    """
    width, height, channels = int(width), int(height), int(channels)
    if not (1 <= width <= PNG_MAX_SIZE and 1 <= height <= PNG_MAX_SIZE):
        raise ValueError(f"png_file writes 1 .. {PNG_MAX_SIZE} rows and columns, got {width} x {height}")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 3 (RGB) or 1 (grey), got {channels}")
    exif_bytes = bytes(exif_bytes)
    if exif_bytes.startswith(b"Exif\x00\x00"):
        exif_bytes = exif_bytes[6:]
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return b"".join((PNG_SIGNATURE, _png_chunk(b"IHDR", ihdr), _png_chunk(b"eXIf", exif_bytes) if exif_bytes else b"",
                     _png_chunk(b"IDAT", bytes(idat_stream), idat_crc), _png_chunk(b"IEND", b"")))


# ---- JPEG: what a decoder needs of a file before its scan (the device decodes the scan: rfx_jpeg_decode_u8) -------------------
class JpegInfo(T.NamedTuple):
    """`jpeg_parse`'s result.  `qtables`: (2, 64) uint16 in natural order, the luma component's table and the chroma components';
    `huffman`: (4, 272) uint8, BITS[16] + HUFFVAL[256] of the luma DC, luma AC, chroma DC and chroma AC tables; `scan`: the byte
    range of the entropy-coded data, after the SOS header and up to (not including) the marker that ends it; `exif`: the APP1
    payload as Pillow keeps it in `info["exif"]` (b"" when the file has none).  Fields the file does not reach are None / 0."""
    width: int
    height: int
    qtables: T.Optional[np.ndarray]
    huffman: T.Optional[np.ndarray]
    scan: T.Tuple[int, int]
    exif: bytes
    ok_for_device: bool
    reason: str


_JPEG_SCAN_END = re.compile(rb"\xff[^\x00]")
_JPEG_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
                   0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic coding",
                   0xCA: "progressive, arithmetic coding", 0xCB: "lossless, arithmetic coding", 0xCD: "differential, arithmetic coding",
                   0xCE: "differential progressive, arithmetic coding", 0xCF: "differential lossless, arithmetic coding"}


def jpeg_parse(data: bytes) -> JpegInfo:
    """
    Walks the markers of a JPEG file up to the end of its first scan.  `ok_for_device` says whether rfx_jpeg_decode_u8 takes the
    file - 8-bit baseline (SOF0), three components Y Cb Cr sampled 2x2, 1x1, 1x1, one interleaved scan with Cb and Cr on the same
    tables, 8-bit quantisation tables, no restart interval - and `reason` why not: progressive and other processes, greyscale,
    CMYK, other subsamplings, restart markers, further scans, an Adobe marker (it may declare RGB), a file that ends without
    EOI, and any marker structure that does not parse.  Never raises for `bytes`.
    """
    data = bytes(data)
    width = height = 0
    exif = b""
    qt: T.Dict[int, np.ndarray] = {}
    ht: T.Dict[int, np.ndarray] = {}

    def result(reason: str, qtables: T.Any = None, huffman: T.Any = None, scan: T.Tuple[int, int] = (0, 0)) -> JpegInfo:
        return JpegInfo(width, height, qtables, huffman, scan, exif, not reason, reason)

    if data[:2] != b"\xff\xd8":
        return result("not a JPEG: no SOI")
    natural = np.asarray(JPEG_NATURAL_ORDER)
    problems: T.List[str] = []  # what keeps the file on the host, found before the scan
    frame: T.Optional[T.List[T.Tuple[int, int, int]]] = None  # (id, sampling, table) of every component
    at, n = 2, len(data)
    while True:
        if at + 2 > n or data[at] != 0xFF:
            return result("malformed: no marker where one must be")
        marker = data[at + 1]
        if marker == 0xFF:  # a fill byte
            at += 1
            continue
        if marker == 0x01 or 0xD0 <= marker <= 0xD7:
            at += 2
            continue
        if marker == 0xD9:
            return result("malformed: EOI before any scan")
        if at + 4 > n:
            return result("malformed: truncated marker segment")
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if length < 2 or at + 2 + length > n:
            return result("malformed: marker segment passes the end of the file")
        seg = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xE1 and seg[:6] == b"Exif\0\0":
            exif = exif + seg[6:] if exif else seg  # (Pillow joins the payloads of a split EXIF)
        elif marker == 0xEE and seg[:5] == b"Adobe":
            problems.append("an Adobe marker: the colour transform is the host's to decide")
        elif marker == 0xDB:
            while seg:
                pq, tq = seg[0] >> 4, seg[0] & 15
                if pq > 1 or tq > 3 or len(seg) < 1 + 64 * (pq + 1):
                    return result("malformed: DQT")
                if pq:
                    problems.append("a 16-bit quantisation table")
                    seg = seg[129:]
                    continue
                table = np.zeros(64, np.uint16)
                table[natural] = np.frombuffer(seg, np.uint8, 64, 1)
                qt[tq] = table
                seg = seg[65:]
        elif marker == 0xC4:
            while seg:
                if len(seg) < 17:
                    return result("malformed: DHT")
                count = sum(seg[1:17])
                if (seg[0] >> 4) > 1 or (seg[0] & 15) > 3 or count > 256 or len(seg) < 17 + count:
                    return result("malformed: DHT")
                code = 0
                for length_bits, codes in enumerate(seg[1:17], 1):
                    code = (code + codes) << 1
                    if code > (2 << length_bits):
                        return result("malformed: DHT is no prefix code")
                table = np.zeros(272, np.uint8)
                table[:16 + count] = np.frombuffer(seg, np.uint8, 16 + count, 1)
                ht[seg[0]] = table
                seg = seg[17 + count:]
        elif marker == 0xDD:
            if len(seg) != 2:
                return result("malformed: DRI")
            if seg != b"\0\0":
                problems.append("a restart interval")
        elif marker == 0xC0 or marker in _JPEG_SOF_NAMES:
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5] or frame is not None:
                return result("malformed: SOF")
            height, width = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(seg[5])]
            if marker != 0xC0:
                problems.append(f"not baseline: {_JPEG_SOF_NAMES[marker]}")
            elif seg[0] != 8:
                problems.append(f"{seg[0]}-bit samples")
            if len(frame) == 1:
                problems.append("greyscale")
            elif len(frame) != 3:
                problems.append(f"{len(frame)} components")
            elif [c[1] for c in frame] != [0x22, 0x11, 0x11]:
                problems.append("a subsampling other than 4:2:0")
            elif [c[0] for c in frame] != [1, 2, 3]:
                problems.append("component ids other than 1, 2, 3: the colour space is the host's to decide")
            if width == 0 or height == 0:
                problems.append("an empty frame or a DNL height")
        elif marker == 0xDA:
            break
    if frame is None:
        return result("malformed: a scan before any frame")
    start = at
    found = _JPEG_SCAN_END.search(data, start)
    end = found.start() if found else n
    if problems:
        return result(problems[0], scan=(start, end))
    if len(seg) != 10 or seg[0] != 3 or [seg[1], seg[3], seg[5]] != [1, 2, 3]:
        return result("a scan that does not interleave the three components", scan=(start, end))
    if seg[7:10] != bytes([0, 63, 0]):
        return result("a scan that is not a whole sequential one", scan=(start, end))
    if seg[4] != seg[6] or frame[1][2] != frame[2][2]:
        return result("Cb and Cr on different tables", scan=(start, end))
    selectors = (seg[2] >> 4, 0x10 | (seg[2] & 15), seg[4] >> 4, 0x10 | (seg[4] & 15))
    if any(s not in ht for s in selectors) or frame[0][2] not in qt or frame[1][2] not in qt:
        return result("malformed: the scan names a table the file does not define", scan=(start, end))
    if found is None:
        return result("the file ends without EOI", scan=(start, end))
    if found.group()[1] != 0xD9:
        what = "restart markers" if 0xD0 <= found.group()[1] <= 0xD7 else "a marker other than EOI after the first scan"
        return result(what, scan=(start, end))
    return result("", np.stack([qt[frame[0][2]], qt[frame[1][2]]]), np.stack([ht[s] for s in selectors]), (start, end))


# ---- PNG: what a decoder needs of a file around its IDAT payloads (the device inflates and unfilters them: rfx_png_decode_u8) ----
class PngInfo(T.NamedTuple):
    """`png_parse`'s result.  `channels`: bytes per pixel of the filtered rows (1, 3, 1, 4 for colour types 0, 2, 3, 6; 0 for any
    other); `palette`: (256, 3) uint8, the PLTE's entries and zeros behind them; `idat`: the byte ranges of the IDAT payloads in
    file order (their concatenation is the zlib stream); `exif`: the eXIf payload (b"" when the file has none)."""
    width: int
    height: int
    color_type: int
    channels: int
    palette: np.ndarray
    palette_entries: int
    idat: T.Tuple[T.Tuple[int, int], ...]
    exif: bytes
    ok_for_device: bool
    reason: str


_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 6: 4}
_PNG_EXIF_TEXT_KEY = b"Raw profile type exif"


def png_parse(data: bytes) -> PngInfo:
    """
    Walks the chunks of a PNG file.  `ok_for_device` says whether rfx_png_decode_u8 takes the file - IHDR first with bit depth 8,
    colour type 0, 2, 3 or 6, no interlace; every chunk's CRC-32 right; the IDAT chunks consecutive; PLTE before IDAT for colour
    type 3; IEND present - and `reason` why not: other depths, grey with alpha, Adam7, APNG chunks, an unknown critical chunk, an
    EXIF kept in a text chunk (Pillow's `getexif` reads it, this parser does not), a CRC mismatch, a truncated file, not a PNG.
    tRNS, gAMA, sRGB, iCCP, pHYs and other text chunks do not change what `convert("RGB")` returns and are skipped.  Never raises
    for `bytes`.
    """
    data = bytes(data)
    width = height = color_type = 0
    palette = np.zeros((256, 3), dtype=np.uint8)
    entries = 0
    idat: T.List[T.Tuple[int, int]] = []
    exif = b""

    def result(reason: str) -> PngInfo:
        return PngInfo(width, height, color_type, _PNG_CHANNELS.get(color_type, 0), palette, entries, tuple(idat), exif, not reason, reason)

    if data[:8] != PNG_SIGNATURE:
        return result("not a PNG: no signature")
    problems: T.List[str] = []  # what keeps the file on the host, in file order
    at, n = 8, len(data)
    first, seen_idat, idat_closed, seen_plte, seen_iend, exif_text = True, False, False, False, False, False
    while not seen_iend:
        if at + 12 > n:
            return result("truncated: the file ends before IEND")
        length = struct.unpack(">I", data[at:at + 4])[0]
        kind = data[at + 4:at + 8]
        if length >= 1 << 31 or at + 12 + length > n:
            return result(f"truncated: the file ends inside a {kind!r} chunk")
        payload = data[at + 8:at + 8 + length]
        if zlib.crc32(data[at + 4:at + 8 + length]) != struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0]:
            problems.append(f"CRC mismatch in a {kind!r} chunk")
        if first:
            if kind != b"IHDR" or length != 13:
                return result("malformed: IHDR is not the first chunk")
            width, height, depth, color_type, compression, filter_method, interlace = struct.unpack(">IIBBBBB", payload)
            if depth != 8:
                problems.append(f"bit depth {depth}")
            if color_type == 4:
                problems.append("colour type 4 (grey with alpha)")
            elif color_type not in _PNG_CHANNELS:
                problems.append(f"colour type {color_type}")
            if compression != 0 or filter_method != 0:
                problems.append("an unknown compression or filter method")
            if interlace != 0:
                problems.append("Adam7 interlace")
            if not (1 <= width <= PNG_MAX_SIZE and 1 <= height <= PNG_MAX_SIZE):
                problems.append(f"{width} x {height} pixels")
            first = False
        elif kind == b"IHDR":
            problems.append("a second IHDR")
        elif kind == b"IDAT":
            if idat_closed:
                problems.append("IDAT chunks that are not consecutive")
            if color_type == 3 and not seen_plte:
                problems.append("colour type 3 without PLTE before IDAT")
            seen_idat = True
            idat.append((at + 8, at + 8 + length))
        elif kind == b"PLTE":
            if seen_idat or seen_plte or length % 3 or length > 768 or length == 0:
                problems.append("a PLTE chunk out of place or of a wrong length")
            else:
                entries = length // 3
                palette[:entries] = np.frombuffer(payload, dtype=np.uint8).reshape(entries, 3)
            seen_plte = True
        elif kind == b"IEND":
            seen_iend = True
        elif kind in (b"acTL", b"fcTL", b"fdAT"):
            problems.append("APNG chunks")
        elif kind == b"eXIf":
            exif = payload
        elif kind in (b"tEXt", b"zTXt", b"iTXt"):
            if payload.split(b"\x00", 1)[0] == _PNG_EXIF_TEXT_KEY:
                exif_text = True
        elif not kind[0] & 0x20:
            problems.append(f"an unknown critical chunk {kind!r}")
        if seen_idat and kind != b"IDAT":
            idat_closed = True
        at += 12 + length
    if not idat:
        problems.append("no IDAT chunk")
    if exif_text and not exif:
        problems.append("EXIF in a text chunk (Raw profile type exif)")
    return result(problems[0] if problems else "")
