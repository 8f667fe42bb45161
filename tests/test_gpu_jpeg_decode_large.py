"""
The JPEG decoder's kernels (csrc/rfx_jpeg_dec.hip) where tests/test_gpu_jpeg_decode.py and tests/test_gpu_jpeg_decode_seams.py do
not reach: the cases L1-L6 of tests/test_jpeg_decode_batch_cpu.py, whose builders assert their edges on the CPU.
  L1, L2  a scan of more than 64 * 256 chunks of 16 bytes - the second trip of jpd_unstuff_kernel's grid-stride loop, its cap of
          64 workgroups, short images idling through the long image's grid - and of more than eight entropy groups: the carry, the
          block base and the reload of the LDS bits from one group to the next.  L1: Pillow's file of 384 x 384 noise at quality
          100, first and last of three; L2: the writer's stress blocks, longer than a subsequence, in every group.
  L3      64 images in one call, with tables that differ and damaged scans at places 0, 31 and 63: every image's pixels and
          status are those of its own one-image call; 64 device-encoded tiles back through images_from_jpeg_bytes.
  L4      status 2 (kJpdBadTable), which only a C ABI caller reaches: the entropy kernel's early return flags that image alone.
  L5      a scan longer than kJpdMaxScanBytes is refused before anything is launched.
  L6      a stream of the caller's, the default stream, a cleared workspace: the same bits.
  S1      scans with several causes of a status: the largest is reported (the device did; the host emulator reported the first,
          which the 64-image case showed on its first device run).
Stages are compared as in the seams file: ulen and the unstuffed bytes, then the coefficients, then the pixels, then the statuses.
The reference of a Pillow file's coefficients is the host emulator's (whose pixels of the same file are Pillow's); where the
emulator cannot be compiled, stages 1 and 2 are left out with a message and the pixels and statuses are still checked.
"""
import numpy as np
import pytest
import torch

from jpeg_decode_batch_cases import BAD_TABLES, Decoded, L3_PLACES, build_large, check_stages, emu, emu_batch, emulator_blocks, layout, one_image
from jpeg_decode_cases import _conv, _three, pillow_pixels

pytestmark = pytest.mark.gpu

TAIL = 24  # bytes of 0x00 behind offsets[N] in the tensor: not the scans'


def _emulator():
    try:
        return emu()
    except Exception as e:  # no host compiler here
        print("host emulator not available:", e)
        return None


def device_decode(c, fill=0xA5, stream=None) -> Decoded:
    """one call of rfx_jpeg_decode_u8 with tensors the test owns.  fill: what the workspace holds before.  stream: a
    torch.cuda.Stream on which every tensor of the call is produced and the call runs; None: the default stream."""
    from riffusion import _hip

    lib = _hip.load_library()
    off, N = c.offsets, len(c.scans)
    need = lib.rfx_jpeg_decode_workspace_bytes(N, c.H, c.W, int(off[-1] - off[0]))
    assert need > 0
    with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
        scans = torch.from_numpy(np.frombuffer(c.buffer(tail=TAIL), np.uint8).copy()).cuda()
        assert scans.numel() == off[-1] + TAIL and scans.data_ptr() % 16 == 0
        d_off = torch.from_numpy(off.copy()).cuda()
        qt = torch.from_numpy(np.ascontiguousarray(c.qtables).view(np.int16).copy()).cuda()
        huff = torch.from_numpy(np.ascontiguousarray(c.huffman)).cuda()
        rgb = torch.zeros((N, c.H, c.W, 3), dtype=torch.uint8, device="cuda")
        status = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        workspace = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        rc = lib.rfx_jpeg_decode_u8(scans.data_ptr(), off.ctypes.data, d_off.data_ptr(), N, c.H, c.W, qt.data_ptr(), huff.data_ptr(), rgb.data_ptr(),
                                    status.data_ptr(), workspace.data_ptr(), stream.cuda_stream if stream is not None else None)
        assert rc == 0, lib.rfx_last_error()
        (stream if stream is not None else torch.cuda.default_stream()).synchronize()
        return Decoded(status.cpu().numpy(), rgb.cpu().numpy(), workspace.cpu().numpy())


def check_device(c, got):
    """the stages in their order; the first that differs is named"""
    N = len(c.scans)
    host = None
    if _emulator() is not None:
        host = emu_batch(c)
        ref = emulator_blocks(c, host)
        assert got.workspace.size == layout(N, c.H, c.W, int(c.offsets[-1] - c.offsets[0])).total
        check_stages(ref, got, stages=("unstuffed",), who="device")
        check_stages(ref, got, stages=("coef",), who="device")
    else:
        print(c.name, ": stages 1 and 2 not compared: no host emulator for the layout")
    for n in range(N):
        if c.status[n] != 0:
            continue  # (its pixels are unspecified)
        if c.files[n] is not None:
            assert np.array_equal(got.rgb[n], pillow_pixels(c.files[n])), f"{c.name}: device: IDCT / pixels stage: image {n} differs from Pillow"
        elif host is not None:
            assert np.array_equal(got.rgb[n], host.rgb[n]), f"{c.name}: device: IDCT / pixels stage: image {n} differs from the host emulator"
    assert got.status.tolist() == c.status, f"{c.name}: device: status"
    if host is not None:
        assert got.status.tolist() == host.status.tolist(), f"{c.name}: device: status differs from the host emulator's"


@pytest.mark.parametrize("name", ["L1_first", "L1_last", "L2", "S1"])
def test_long_scans_and_the_largest_of_several_causes(name):
    """L1, L2 (the builder asserts more than 64 * 256 * 16 scan bytes and more than 8 * 256 subsequences beside a short image).
    The reference of L2's stress pixels is the host emulator, of its coefficients the writer's blocks.  S1: scans with two causes
    of a status each; the largest is reported, as include/rfx.h says."""
    c = build_large(name)
    check_device(c, device_decode(c))


@pytest.fixture(scope="module")
def l3_whole():
    c = build_large("L3")
    return c, device_decode(c)


def test_64_images_the_damaged_ones_flagged_and_the_sound_ones_as_pillow(l3_whole):
    c, whole = l3_whole
    assert len(c.scans) == 64 and np.flatnonzero(whole.status).tolist() == list(L3_PLACES), whole.status
    for n in range(64):
        if n not in L3_PLACES:
            assert np.array_equal(whole.rgb[n], pillow_pixels(c.files[n])), n
    if _emulator() is not None:
        assert whole.status.tolist() == emu_batch(c).status.tolist()


def test_an_image_decodes_the_same_alone_and_at_any_place_of_64(l3_whole):
    """pixels and status, byte for byte, the damaged images' included"""
    c, whole = l3_whole
    for n in range(64):
        single = device_decode(one_image(c, n))
        assert single.status[0] == whole.status[n], (n, single.status, whole.status[n])
        assert np.array_equal(single.rgb[0], whole.rgb[n]), n


def test_64_device_encoded_tiles_in_one_call_decode_as_pillow_decodes_them():
    conv = _conv()
    contents = _three(64, 96)
    x = np.stack([contents[n % 3] ^ np.uint8(n) for n in range(64)])  # 64 different tiles of 64 x 96
    files = conv.jpeg_bytes_from_images(x)
    assert len(files) == 64 and len(set(files)) == 64
    plan = conv.converter._plan()
    calls, decode = [], plan.jpeg_decode
    plan.jpeg_decode = lambda scans, *a: (calls.append(len(scans)), decode(scans, *a))[1]
    try:
        assert conv.converter._plan() is plan
        tiles, _ = conv.images_from_jpeg_bytes(files, return_device=True)
    finally:
        del plan.jpeg_decode
    assert calls == [64]
    assert isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.shape == (64, 64, 96, 3)
    for t, f in zip(tiles.cpu().numpy(), files):
        assert np.array_equal(t, pillow_pixels(f))


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("kind", BAD_TABLES)
def test_a_bad_huffman_table_flags_its_image_alone(kind, which):
    """L4: the middle of three images has table `which` (DC0 AC0 DC1 AC1) replaced; statuses [0, 2, 0], the outer images exact"""
    c = build_large(f"L4_{kind}_{which}")
    assert c.status == [0, 2, 0]
    check_device(c, device_decode(c))


def test_a_scan_longer_than_the_limit_is_refused_before_launch():
    from riffusion import _hip

    lib = _hip.load_library()
    limit = (1 << 28) - 64  # kJpdMaxScanBytes
    buf = torch.full((4096,), 0x5C, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    off = np.array([0, limit + 1], np.int64)
    rc = lib.rfx_jpeg_decode_u8(p, off.ctypes.data, p + 2048, 1, 8, 8, p + 1024, p + 1024, p + 512, p + 3072, p, None)
    assert rc == -4 and b"2^28 - 64" in lib.rfx_last_error()  # RFX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == 0x5C).all())  # nothing ran
    assert lib.rfx_jpeg_decode_workspace_bytes(1, 8, 8, 1 << 28) == 0
    assert lib.rfx_jpeg_decode_workspace_bytes(1, 8, 8, limit) > limit  # (the size only: nothing of that size is launched)
    assert lib.rfx_jpeg_decode_workspace_bytes(1, 8, 8, limit + 1) == 0 and lib.rfx_jpeg_decode_workspace_bytes(2, 8, 8, 2 * limit) > 2 * limit


def test_a_stream_of_the_caller_s_and_a_cleared_workspace_give_the_same_bits():
    c = build_large("L3_sound")
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0 and side != torch.cuda.default_stream()
    on_side, on_default, cleared = device_decode(c, stream=side), device_decode(c), device_decode(c, fill=0x00)
    assert not on_side.status.any()
    for other in (on_default, cleared):
        assert np.array_equal(on_side.status, other.status) and np.array_equal(on_side.rgb, other.rgb)
    for n in range(64):
        assert np.array_equal(on_side.rgb[n], pillow_pixels(c.files[n])), n
