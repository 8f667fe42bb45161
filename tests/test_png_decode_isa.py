"""
What the compiler made of the PNG decode kernels (csrc/rfx_png_dec.hip), read from the descriptors hipcc emits for gfx950 (no GPU
needed; tools/isa_resources.py does the reading): neither kernel uses scratch - the decode tables, the window and the rows, which
are indexed by data, live in LDS, not in private memory - and each one's LDS is what csrc/rfx_png_dec_core.h states for it (the
inflate's shared structure and the 4 KiB staging buffer of the stream beside it; the unfilter's shared structure).  The check is
the `.amdhsa_private_segment_fixed_size` and `.amdhsa_group_segment_fixed_size` fields; the instruction text is not searched.
"""
import os
import sys

import pytest

import png_decode_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "riffusion-hobby_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ("png_inflate_kernel", "png_unfilter_kernel")
STAGE_BYTES = 4096  # rfx_png_dec.hip's kPngdStageBytes


@pytest.fixture(scope="module")
def rows():
    import isa_resources

    return isa_resources.kernels_of(os.path.join(CSRC, "rfx_png_dec.hip"))


def test_every_kernel_is_there_once(rows):
    names = [r["kernel"] for r in rows]
    for k in KERNELS:
        assert sum((k + "(") in n for n in names) == 1, (k, names)
    assert len(rows) == len(KERNELS)


def test_no_kernel_uses_scratch(rows):
    for r in rows:
        assert r["scratch_bytes"] == 0, r["kernel"]


def test_lds_is_what_the_core_header_states(rows):
    by = {k: next(r for r in rows if (k + "(") in r["kernel"]) for k in KERNELS}
    lib = C.emu()
    inflate, unfilter = lib.emu_png_dec_inflate_shared_bytes(), lib.emu_png_dec_unfilter_shared_bytes()
    assert 32768 < inflate < 32768 + 6144  # the window and a few KiB of tables
    assert by["png_inflate_kernel"]["static_lds_bytes"] == inflate + STAGE_BYTES
    assert by["png_unfilter_kernel"]["static_lds_bytes"] == unfilter < 2 * lib.emu_png_dec_seg_bytes() + 1024
    # both leave a CU's 160 KiB room for several workgroups
    assert all(r["static_lds_bytes"] <= 48 * 1024 for r in rows)
