"""
What the compiler made of the int16 front-end kernels (csrc/rfx_pcm_in.hip), read from the ISA hipcc emits for gfx950 (no GPU
needed; tools/isa_resources.py does the reading): both kernels, in each of their four channel forms, keep their runs in
registers - no scratch - use no LDS, and the resample kernel stores its runs as 16-byte groups.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "riffusion-hobby_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    import isa_resources

    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *isa_resources.FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "rfx_pcm_in.hip")], check=True,
                       capture_output=True, cwd=CSRC)
        return open(out).read()


def kernels(text, pattern):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S) if re.search(pattern, m.group(1))}


def field(body, key):
    return int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", body).group(1))


@pytest.mark.parametrize("pattern", ["pcm_ratecv_kernel", "pcm_clips_kernel"])
def test_kernels_hold_no_scratch_and_no_lds(asm, pattern):
    found = kernels(asm, pattern)
    assert len(found) == 4, sorted(found)  # (C_in, C_out) in {1, 2}^2
    for sym, body in found.items():
        assert field(body, "private_segment_fixed_size") == 0, sym
        assert field(body, "group_segment_fixed_size") == 0, sym
        code = asm[asm.index(sym + ":"):]
        code = code[:code.index("s_endpgm")]
        assert not re.search(r"^\s+scratch_", code, re.M), sym


def test_resample_kernel_stores_its_runs_as_16_byte_groups(asm):
    for sym in kernels(asm, "pcm_ratecv_kernel"):
        code = asm[asm.index(sym + ":"):]
        code = code[:code.index("s_endpgm")]
        wide = re.findall(r"^\s+global_store_dwordx4", code, re.M)
        c_out = int(re.search(r"pcm_ratecv_kernelILi[12]ELi([12])E", sym).group(1))
        assert len(wide) == c_out, (sym, len(wide))  # 8 frames of 2 * C_out bytes
