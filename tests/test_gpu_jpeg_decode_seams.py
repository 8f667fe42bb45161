"""
The JPEG decoder's kernels (csrc/rfx_jpeg_dec.hip) on the cases of tests/test_jpeg_decode_batch_cpu.py: scans from
tests/jpeg_scan_writer.py whose codewords, stuffed bytes and ends fall on the kernels' seams - chunks shared by images, any
offsets[0], the 1024-chunk pass of the unstuff scan, subsequences and groups of the entropy kernel, the 1024-MCU pass of the DC
scan.  rfx_jpeg_decode_u8 is called through the C ABI with tensors the test owns, so that it chooses offsets[0] and the bytes
around the scans and keeps the workspace; after one synchronisation the workspace is compared in the order of the stages, whole
arrays, no tolerance, and the first mismatch names its stage:
  1. ulen[n] and every image's unstuffed region against the writer's unstuffed bytes;
  2. the coefficients against the writer's blocks (natural order, DC as values): the entropy and DC-scan kernels against a
     reference that shares no code with the decoder;
  3. the pixels.  Picture inputs: against Pillow's decode of the file.  Stress inputs (every AC term the largest of its size,
     Huffman tables no encoder writes): against the HOST EMULATOR's pixels - their coefficients are not ones a real image reaches,
     libjpeg-turbo's SIMD IDCT saturates where its C routine masks (rfx_jpeg_dec_core.h), so Pillow is no defined reference for
     them; the coefficient comparison of stage 2 is the strong one there;
  4. the statuses.
The offsets of the regions come from the host emulator (emu_jpeg_dec_layout: the device's own layout function, compiled for the
host).  Where the emulator cannot be compiled, stages 1 and 2 and the stress pixels are left out with a message; the picture
pixels and the statuses are still checked.
"""
import numpy as np
import pytest
import torch

from jpeg_decode_batch_cases import BUILDERS, Decoded, build_case, check_stages, emu, emu_batch, layout
from jpeg_decode_cases import pillow_pixels

pytestmark = pytest.mark.gpu

TAIL = 24  # bytes of 0x00 behind offsets[N] in the tensor: not the scans'


def _emulator():
    try:
        return emu()
    except Exception as e:  # no host compiler here
        print("host emulator not available:", e)
        return None


def device_decode(c) -> Decoded:
    from riffusion import _hip

    lib = _hip.load_library()
    off, N = c.offsets, len(c.scans)
    total = int(off[-1] - off[0])
    need = lib.rfx_jpeg_decode_workspace_bytes(N, c.H, c.W, total)
    assert need > 0
    scans = torch.from_numpy(np.frombuffer(c.buffer(tail=TAIL), np.uint8).copy()).cuda()
    assert scans.numel() == off[-1] + TAIL and scans.data_ptr() % 16 == 0
    d_off = torch.from_numpy(off.copy()).cuda()
    qt = torch.from_numpy(np.ascontiguousarray(c.qtables).view(np.int16).copy()).cuda()
    huff = torch.from_numpy(np.ascontiguousarray(c.huffman)).cuda()
    rgb = torch.zeros((N, c.H, c.W, 3), dtype=torch.uint8, device="cuda")
    status = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")  # nothing relies on a cleared workspace
    rc = lib.rfx_jpeg_decode_u8(scans.data_ptr(), off.ctypes.data, d_off.data_ptr(), N, c.H, c.W, qt.data_ptr(), huff.data_ptr(), rgb.data_ptr(),
                                status.data_ptr(), workspace.data_ptr(), None)
    assert rc == 0, lib.rfx_last_error()
    torch.cuda.synchronize()
    return Decoded(status.cpu().numpy(), rgb.cpu().numpy(), workspace.cpu().numpy())


@pytest.mark.parametrize("name", list(BUILDERS))
def test_device_stage_outputs_equal_the_writer(name):
    """the reference of the stress images' pixels is the host emulator, not Pillow: see the module's docstring"""
    c = build_case(name)  # (asserts that the case reaches its edge)
    got = device_decode(c)
    N = len(c.scans)
    host = None
    if _emulator() is not None:
        assert got.workspace.size == layout(N, c.H, c.W, int(c.offsets[-1] - c.offsets[0])).total
        check_stages(c, got, stages=("unstuffed",), who="device")
        check_stages(c, got, stages=("coef",), who="device")
        host = emu_batch(c)
    else:
        print(name, ": stages 1 and 2 not compared: no host emulator for the layout")
    for n in range(N):
        if c.status[n] != 0:
            continue
        if c.files[n] is not None:
            assert np.array_equal(got.rgb[n], pillow_pixels(c.files[n])), f"{name}: device: IDCT / pixels stage: image {n} differs from Pillow"
        elif host is not None:
            assert np.array_equal(got.rgb[n], host.rgb[n]), f"{name}: device: IDCT / pixels stage: image {n} differs from the host emulator"
    assert got.status.tolist() == c.status, f"{name}: device: status"


@pytest.mark.parametrize("off0", [16, 5, 37])
def test_first_offset_changes_nothing(off0):
    base, moved = device_decode(build_case("U4_0")), device_decode(build_case(f"U4_{off0}"))
    assert np.array_equal(base.status, moved.status) and np.array_equal(base.rgb[:2], moved.rgb[:2])
