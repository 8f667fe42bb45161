"""
What the compiler made of the chirp-z kernels (csrc/rfx_czt.hip), read from the ISA hipcc emits for gfx950 (no GPU needed), as
tests/test_isa_resources.py does for the other engines.  A kernel holds the forward and the inverse passes of its convolution - the
Griffin-Lim kernel two of each - and is given 256 VGPRs (two waves per SIMD) so that none of it lives in scratch memory:
  * every forward kernel and the Griffin-Lim kernels of the 2 / 3 / 5 / 7 radix classes: not one scratch instruction;
  * the Griffin-Lim analysis kernels of the radix-11 / 13 class (O(R^2) butterflies, all 256 registers in use): three dwords parked
    ahead of the passes and re-loaded once each - six scratch instructions among 57 000, 16 bytes;
  * no kernel goes past 256 VGPRs or uses static LDS (the buffer is dynamic, sized by czt_lds_bytes).
The initial-synthesis kernels (mode 0) reserve 20 - 36 bytes of private segment for an indexed local array and never touch it with a
scratch instruction.  Three compiles side by side, one radix class each (five kernels).
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
def kernels():
    import isa_resources

    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(3) as ex:  # one radix class per compile (RFX_CZT_CLASS), the three side by side
        rows = [r for rs in ex.map(lambda c: isa_resources.kernels_of(os.path.join(CSRC, "rfx_czt.hip"), [f"-DRFX_CZT_CLASS={c}"]), (5, 7, 13)) for r in rs]
    return {r["kernel"].split("(")[0].replace("void rfx::", ""): r for r in rows}


def test_every_mode_and_class_is_there(kernels):
    want = {f"czt_stft_kernel<{m}, {c}>" for m in (0, 1) for c in (5, 7, 13)} | {f"czt_gl_kernel<{m}, {c}>" for m in (0, 1, 2) for c in (5, 7, 13)}
    assert set(kernels) == want


def test_registers_and_scratch(kernels):
    for name, r in sorted(kernels.items()):
        print(f"{name}: {r['vgpr']} VGPRs, {r['scratch_bytes']} B private segment, {r['scratch_instructions_static']} scratch instructions of "
              f"{r['instructions_static']}")
        assert r["vgpr"] <= 256 and r["static_lds_bytes"] == 0, name
        heavy = name in ("czt_gl_kernel<1, 13>", "czt_gl_kernel<2, 13>")
        if heavy:
            assert r["scratch_instructions_static"] <= 6 and r["scratch_bytes"] <= 16, name
        else:
            assert r["scratch_instructions_static"] == 0, name
            assert r["scratch_bytes"] == 0 or (name.startswith("czt_gl_kernel<0") and r["scratch_bytes"] <= 36), name
