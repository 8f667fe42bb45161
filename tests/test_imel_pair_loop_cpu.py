"""
The InverseMelScale wave kernel's SGD step with the chunks' scalar chains paired (rfx_imel_wave.hip, imel_wave_kernel): what the
compiler made of it, read from the ISA hipcc emits for gfx950 (no GPU needed).  The per-group scalars of chunks 2j and 2j + 1
(A / B, residual, loss terms, gradient line) run as one v_pk_*_f32; the shifts and the pair tails stay plain.  Held here, for both
instantiations (unit form and both weights):
  * no scratch, at most 256 VGPRs (two waves per SIMD);
  * the step loop issues at most 260 VALU instructions (305 before the pairing), at least 176 of them packed;
  * at most 4 plain v_mov_b32 in the loop: the pairing must not come back as register shuffles around the 16 DPP shifts.
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
SYMBOLS = {"unit form": "_ZN3rfx16imel_wave_kernelILb1EEEvNS_8ImelArgsE", "both weights": "_ZN3rfx16imel_wave_kernelILb0EEEvNS_8ImelArgsE"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    import isa_resources

    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *isa_resources.FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "rfx_imel_wave.hip")], check=True,
                       capture_output=True, cwd=CSRC)
        return open(out).read()


def loop_lines(text, symbol):
    """the instruction lines of the SGD step loop, found the way tools/isa_mix.py finds it"""
    s = text.index(symbol + ":")
    body = text[s:text.index("s_endpgm", s)].split("\n")
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    loops = [(labels[m.group(1)], i) for i, l in enumerate(body) for m in [re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)]
             if m and m.group(1) in labels and labels[m.group(1)] < i]
    packed = lambda ab: sum(1 for l in body[ab[0]:ab[1] + 1] if re.match(r"\s+v_pk", l))
    most = max(packed(ab) for ab in loops)
    a, b = min((ab for ab in loops if packed(ab) == most), key=lambda ab: ab[1] - ab[0])
    return [l.split()[0] for l in body[a:b + 1] if re.match(r"\s+[a-z]", l) and not l.strip().startswith(".")]


def kernel_field(text, symbol, name):
    body = re.search(r"\.amdhsa_kernel " + re.escape(symbol) + r"(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
    return int(re.search(r"\.amdhsa_" + name + r"\s+(\d+)", body).group(1))


@pytest.mark.parametrize("form", sorted(SYMBOLS))
def test_paired_step_loop(asm, form):
    sym = SYMBOLS[form]
    assert kernel_field(asm, sym, "private_segment_fixed_size") == 0
    assert kernel_field(asm, sym, "next_free_vgpr") <= 256
    ops = loop_lines(asm, sym)
    valu = [o for o in ops if o.startswith("v_")]
    packed = [o for o in valu if o.startswith("v_pk_")]
    dpp = [o for o in valu if o.endswith("_dpp")]
    moves = [o for o in valu if o.startswith("v_mov_b32") and not o.endswith("_dpp")]
    print(f"{form}: {len(valu)} VALU ({len(packed)} packed, {len(dpp)} DPP, {len(moves)} moves)")
    assert len(dpp) == 16  # two neighbour shifts per chunk, 32-bit
    assert len(valu) <= 260
    assert len(packed) >= 176
    assert len(moves) <= 4
    assert ops.count("ds_add_f32") == 1  # one LDS add of the step's loss per wave
