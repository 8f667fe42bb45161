"""
What the compiler made of the PNG kernels (csrc/rfx_png.hip), read from the descriptors hipcc emits for gfx950 (no GPU needed;
tools/isa_resources.py does the reading): none of the eight kernels uses scratch - the code builder's tables, which are indexed by
data, live in LDS, not in private memory.  The check is the `.amdhsa_private_segment_fixed_size` field; the instruction text is not
searched.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "riffusion-hobby_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ("png_grey_kernel", "png_filter_kernel", "png_tokens_kernel<false>", "png_tokens_kernel<true>", "png_build_kernel",
           "png_finish_kernel", "png_crc_kernel", "png_copy_kernel")


@pytest.fixture(scope="module")
def rows():
    import isa_resources

    return isa_resources.kernels_of(os.path.join(CSRC, "rfx_png.hip"))


def test_every_kernel_is_there_once(rows):
    names = [r["kernel"] for r in rows]
    for k in KERNELS:
        assert sum(("rfx::" + k + "(") in n for n in names) == 1, (k, names)
    assert len(rows) == len(KERNELS)


def test_no_kernel_uses_scratch(rows):
    for r in rows:
        assert r["scratch_bytes"] == 0, r["kernel"]


def test_lds_is_what_the_kernels_declare(rows):
    by = {k: next(r for r in rows if ("rfx::" + k + "(") in r["kernel"]) for k in KERNELS}
    assert by["png_grey_kernel"]["static_lds_bytes"] == 0 and by["png_copy_kernel"]["static_lds_bytes"] == 0
    # the builder's working storage and the block's codes: a few KiB, many workgroups to a CU
    assert 6000 < by["png_build_kernel"]["static_lds_bytes"] < 8192
    # the packing round's window: 1024 tokens of at most 21 bits
    assert 674 * 4 <= by["png_tokens_kernel<true>"]["static_lds_bytes"] < 4096
    assert by["png_tokens_kernel<false>"]["static_lds_bytes"] < 2048
