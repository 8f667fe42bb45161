"""
CPU checks of the spectral-peak start (include/rfx.h: rfx_peak_start, rfx_start_call_options): Griffin-Lim's initial angles built from
the magnitudes alone.

* The arithmetic of csrc/rfx_peak_core.h, compiled for the host with tests/emu/rfx_peak_emu.cpp and walked as the kernels walk it,
  against the float64 restatement tests/peak_start_oracle.py: every component of every angle within 1e-5.  The bound is derived: the
  decisions (peaks, owners) are float32 compares and agree exactly; the double chain agrees to about 1e-11 turns; what is left is the
  float32 rounding of the fraction (6e-8 turns = 4e-7 rad) and float32 sincos of an argument up to 2 pi (a few 1e-7).
  Default geometry (the specialised slot order) B = 3, T = 37; 8 kHz / 64 filters B = 2, T = 21 (plain frames, and the same through a
  position table).  Inputs: crafted frames that hold every decision case - asserted from the restatement's peak lists - and columns
  100:137 of og_beat.png through the oracle's SGD.
* Quality, on the oracle: with the restatement's start Griffin-Lim's spectral convergence at 0 iterations is below half the random
  start's and at 2 iterations below the random start's, on each of the five seed tiles.
* The layout of the grown options struct against the header, the shorter sizes, every refusal that needs no device, the queries
  without a plan, the CLI flags.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import helpers
import peak_start_inputs as inputs
import peak_start_oracle
from helpers import oracle

EMU_SRC = "rfx_peak_emu.cpp"
SPEC, PLAIN, TABLE = 0, 1, 2
TILES = ["og_beat", "vibes", "agile", "marim", "motorway"]


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_peak_in_bin.argtypes = [i, i, i, vp]
    lib.emu_peak_out_bin.argtypes = [i, i, i, ctypes.POINTER(i)]
    lib.emu_peak_owners.argtypes = [vp, i, vp]
    lib.emu_peak_owners.restype = None
    lib.emu_peak_start.argtypes = [i, vp, vp, i, i, i, i, i, i, i, vp, i]
    lib.emu_peak_start.restype = None
    return lib


@pytest.fixture(scope="module")
def lib():
    from riffusion import _hip

    return _hip.load_library()


def _params(O, **kw):
    from riffusion.spectrogram_params import SpectrogramParams

    return O.params_from(SpectrogramParams(**kw))


def _rows(O, p, golden_dir, B, T):
    """(B, F, T) float32: row 0 crafted, row 1 real magnitudes (og_beat columns 100:137 cut or tiled to T, the SGD at the default
    filterbank only), further rows crafted from another seed; and the crafted row's case table"""
    F = p.n_stft
    crafted, at = inputs.crafted_row(F, T)
    rows = [crafted]
    if p.n_fft == 17640:
        rows.append(inputs.tile_magnitudes(O, p, golden_dir, "og_beat", 100, 137)[0].numpy()[:, :T])
    while len(rows) < B:
        rows.append(inputs.crafted_row(F, T, seed=10 + len(rows))[0])
    return np.ascontiguousarray(np.stack(rows[:B]).astype(np.float32)), at


def _in_map(emu, layout, stride, F, bin_of=None):
    ptr = bin_of.ctypes.data if bin_of is not None else None
    return np.array([emu.emu_peak_in_bin(layout, p, F, ptr) for p in range(stride)])


def _out_map(emu, spec, stride, F):
    cj = ctypes.c_int(0)
    bins, conj = [], []
    for p in range(stride):
        bins.append(emu.emu_peak_out_bin(spec, p, F, ctypes.byref(cj)))
        conj.append(cj.value)
    return np.array(bins), np.array(conj, bool)


def _run_emu(emu, layout, mag, hop, n_fft, stride_in, bin_of=None):
    """the emulator on (B, F, T) magnitudes laid out in `layout`: (angles (B*T, stride_out) complex64, out bins, out conj)"""
    B, F, T = mag.shape
    spec = layout == SPEC
    stride_out = emu.emu_peak_spec_stride() if spec else F + 5
    in_bins = _in_map(emu, layout, stride_in, F, bin_of)
    S = np.full((B * T, stride_in), np.float32(-1e30), np.float32)  # padding the emulator must not read
    frames = mag.transpose(0, 2, 1).reshape(B * T, F)
    S[:, in_bins >= 0] = frames[:, in_bins[in_bins >= 0]]
    out = np.full((B * T, stride_out, 2), np.float32(np.nan), np.float32)
    emu.emu_peak_start(layout, S.ctypes.data, bin_of.ctypes.data if bin_of is not None else None, B, T, stride_in, F, hop, n_fft, int(spec),
                       out.ctypes.data, stride_out)
    bins, conj = _out_map(emu, int(spec), stride_out, F)
    return out[..., 0] + 1j * out[..., 1], bins, conj


def _check_against_restatement(got, bins, conj, want):
    """every position of every frame: padding exactly 0, a bin's every copy within 1e-5 of the restatement (conjugated in conjugate slots)"""
    B, F, T = want.shape
    ref = want.transpose(0, 2, 1).reshape(B * T, F)
    assert not np.isnan(got.real).any() and not np.isnan(got.imag).any()  # every position written
    assert (got[:, bins < 0] == 0).all()
    assert set(bins[bins >= 0]) == set(range(F))
    e = ref[:, bins[bins >= 0]]
    e = np.where(conj[bins >= 0][None, :], e.conj(), e)
    g = got[:, bins >= 0]
    err = max(float(np.abs(g.real - e.real).max()), float(np.abs(g.imag - e.imag).max()))
    print(f"largest component error against the restatement: {err:.2e}")
    assert err <= 1e-5
    return err


def test_emulator_matches_the_restatement_default_geometry(O, emu, golden_dir):
    p = _params(O)
    mag, at = _rows(O, p, golden_dir, 3, 37)
    want, peaks = peak_start_oracle.peak_start(mag, p.hop_length, p.n_fft, details=True)
    inputs.assert_crafted_cases(peaks[0], at, p.n_stft)
    assert min(len(q) for q in peaks[1]) > 0  # the tile row: real magnitudes have peaks in every frame
    got, bins, conj = _run_emu(emu, SPEC, mag, p.hop_length, p.n_fft, emu.emu_peak_spec_stride())
    assert conj.any() and len(bins[bins >= 0]) == 9261  # conjugate slots and the 440 bins stored twice are in the layout
    _check_against_restatement(got, bins, conj, want)
    # the frames without a peak: phase 0 everywhere, (-1)^k
    t = at["zero"]
    g = got[t][bins >= 0]
    assert np.array_equal(g.real, np.where(bins[bins >= 0] % 2 == 1, -1.0, 1.0).astype(np.float32)) and (g.imag == 0).all()


@pytest.mark.parametrize("layout", [PLAIN, TABLE], ids=["plain", "table"])
def test_emulator_matches_the_restatement_8k_64_filters(O, emu, golden_dir, layout):
    p = _params(O, sample_rate=8000, max_frequency=4000, num_frequencies=64)
    assert (p.n_fft, p.hop_length, p.n_stft) == (3200, 80, 1601)
    mag, at = _rows(O, p, golden_dir, 2, 21)
    want, peaks = peak_start_oracle.peak_start(mag, p.hop_length, p.n_fft, details=True)
    inputs.assert_crafted_cases(peaks[0], at, p.n_stft)
    F = p.n_stft
    bin_of, stride_in = None, F + 3
    if layout == TABLE:  # a position table as the row family's: a permutation of the bins with padding in between
        rng = np.random.default_rng(1)
        stride_in = F + 40
        bin_of = np.full(stride_in, -1, np.int32)
        bin_of[rng.permutation(stride_in)[:F]] = rng.permutation(F).astype(np.int32)
    got, bins, conj = _run_emu(emu, layout, mag, p.hop_length, p.n_fft, stride_in, bin_of)
    assert not conj.any()
    _check_against_restatement(got, bins, conj, want)


def test_owners_of_the_emulator_equal_the_restatement_exactly(O, emu):
    """the decisions are exact: on every crafted frame the owner of every bin is the restatement's, bit for bit"""
    F = 1601
    crafted, _ = inputs.crafted_row(F, 21)
    for t in range(crafted.shape[1]):
        m = np.ascontiguousarray(crafted[:, t])
        own = np.zeros(F, np.uint16)
        emu.emu_peak_owners(m.ctypes.data, F, own.ctypes.data)
        want = peak_start_oracle.frame_owners(peak_start_oracle.frame_peaks(m), F)
        assert np.array_equal(np.where(own == 0xFFFF, -1, own.astype(np.int64)), want), t


def test_a_row_depends_on_its_magnitudes_alone(emu):
    F, T = 1601, 21
    a, _ = inputs.crafted_row(F, T)
    b, _ = inputs.crafted_row(F, T, seed=9)
    alone, _, _ = _run_emu(emu, PLAIN, a[None], 80, 3200, F)
    batch, _, _ = _run_emu(emu, PLAIN, np.stack([b, b, a]), 80, 3200, F)
    assert np.array_equal(alone.view(np.uint32), batch[2 * T:].view(np.uint32))


# ---- quality, on the oracle ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def quality(O, golden_dir):
    """per tile: spectral convergence of the oracle's Griffin-Lim from the random and from the peak start at 0 and 2 iterations"""
    p = _params(O)
    out = {}
    for name in TILES:
        S = inputs.tile_magnitudes(O, p, golden_dir, name, 100, 228)
        rand0 = torch.rand(S.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(1234))
        peak0 = torch.from_numpy(peak_start_oracle.peak_start(S.numpy(), p.hop_length, p.n_fft)).to(torch.complex64)
        out[name] = {(kind, n): O.spectral_convergence(O.griffinlim(S, p, angles0=a0, n_iter=n), S, p)
                     for kind, a0 in (("random", rand0), ("peaks", peak0)) for n in (0, 2)}
        print(name, {f"{k[0]}@{k[1]}": round(v, 4) for k, v in out[name].items()})
    return out


@pytest.mark.parametrize("name", TILES)
def test_peak_start_beats_the_random_start_at_few_iterations(quality, name):
    q = quality[name]
    assert q[("peaks", 0)] < 0.5 * q[("random", 0)]
    assert q[("peaks", 2)] < q[("random", 2)]


# ---- rfx_start_call_options: layout and the refusals that need no device ------------------------------------------------------------------

def test_start_options_layout_matches_the_header(repo_root, tmp_path):
    from riffusion import _hip

    exe = emu_build.header_compiles_as_c99(
        tmp_path,
        '#include <stddef.h>\n#include <stdio.h>\n#include "rfx.h"\n'
        "#define O(f) (int)offsetof(rfx_start_call_options, f)\n"
        "int main(void) {\n"
        '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rfx_loop_call_options), (int)sizeof(rfx_start_call_options), O(flags),\n'
        "         O(row_base), O(magnitude_hint), O(reserved), O(d_guide), O(guide_stride), O(guide_samples), O(reserved2), O(d_hold_frames), O(reserved3),\n"
        "         O(d_hold_bins), O(hold_words), O(reserved4), O(loop), O(reserved5), O(start), O(reserved6));\n"
        "  return 0;\n}\n",
        link=True, extra=("-Wextra",))
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, Lp = _hip.RfxStartCallOptions, _hip.RfxLoopCallOptions
    assert got[:2] == [ctypes.sizeof(Lp), ctypes.sizeof(S)] == [88, 96]
    assert got[2:] == [getattr(S, f).offset for f, _ in S._fields_[1:]]
    assert [getattr(S, f).offset for f, _ in Lp._fields_] == [getattr(Lp, f).offset for f, _ in Lp._fields_]  # the loop-size prefix is the loop struct
    assert (S.start.offset, S.reserved6.offset) == (88, 92)


def test_start_options_builder():
    from riffusion import _hip

    g = torch.zeros(3, 50)
    assert isinstance(_hip.call_options(rows=3, row_base=2), _hip.RfxCallOptions)
    assert isinstance(_hip.call_options(rows=3, loop=True), _hip.RfxLoopCallOptions)
    o = _hip.call_options(rows=3, row_base=2, magnitude_hint=5.0, lstsq=True, peak_start=True)
    assert (o.struct_size, o.flags, o.row_base, o.magnitude_hint, o.loop, o.reserved5, o.start, o.reserved6) == (96, 1, 2, 5.0, 0, 0, 1, 0)
    assert (o.d_guide, o.d_hold_frames, o.d_hold_bins) == (None, None, None)
    assert _hip.call_options(rows=3, loop=True, peak_start=True).loop == 1
    for kw in (dict(guide=g), dict(guide=g, hold=torch.zeros(3, 2, dtype=torch.int32)), dict(guide=g, hold_bins=torch.zeros(3, 4, 51, dtype=torch.int32))):
        with pytest.raises(ValueError, match="peak_start together with"):
            _hip.call_options(rows=3, peak_start=True, **kw)
    assert _hip.check_phase_start("random", guide=g) is False and _hip.check_phase_start("peaks", guide=None) is True
    with pytest.raises(ValueError, match="phase_start must be one of"):
        _hip.check_phase_start("peak")
    with pytest.raises(ValueError, match="does not go with guide"):
        _hip.check_phase_start("peaks", angles0=None, guide=g)


def _start(start=1, reserved6=0, d_guide=None, d_pairs=None, d_bins=None, loop=0, size=None):
    from riffusion import _hip

    return _hip.RfxStartCallOptions(ctypes.sizeof(_hip.RfxStartCallOptions) if size is None else size, 0, 0, 0.0, 0.0, d_guide, 100 if d_guide else 0,
                                    100 if d_guide else 0, 0, d_pairs, 0, d_bins, 276 if d_bins else 0, 0, loop, 0, start, reserved6)


def _gl_ex(lib, opt, angles0=None):
    return lib.rfx_griffinlim_ex(None, None, angles0, 0, 1, 41, 0, 0.5, None, None, 0, None, ctypes.byref(opt), None)


@pytest.mark.parametrize("kw,word", [(dict(start=2), b"start must be 0 or 1"), (dict(start=0xFFFFFFFF), b"start must be 0 or 1"), (dict(reserved6=1), b"reserved6"),
                                     (dict(start=0, reserved6=7), b"reserved6"), (dict(d_guide=0x1000), b"d_guide"),
                                     (dict(d_guide=0x1000, d_pairs=0x2000), b"d_hold_frames"), (dict(d_guide=0x1000, d_bins=0x3000), b"d_hold_bins")])
def test_start_options_are_refused_before_any_device_work(lib, kw, word):
    """the options are read before the plan and the buffers are looked at: null everything else, no GPU needed"""
    opt = _start(**kw)
    assert _gl_ex(lib, opt) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_waveform_from_mel_ex(None, None, 1, 41, 1, 0, 1, 0.5, None, None, 0, None, ctypes.byref(opt)) == -1 and word in lib.rfx_last_error()
    assert lib.rfx_audio_from_image_u8_ex(None, None, 1, 41, 0, None, 0, 1, 0.5, 1, None, None, None, 0, None, ctypes.byref(opt)) == -1
    assert word in lib.rfx_last_error()
    assert helpers.queries_refuse(lib, opt, word)


def test_injected_angles_inverse_mel_shorter_structs_and_queries(lib):
    from riffusion import _hip

    # start == 1 together with d_angles0_slots: refused by name, before the plan is looked at
    assert _gl_ex(lib, _start(), angles0=0x4000) == -1 and b"d_angles0_slots" in lib.rfx_last_error()
    assert lib.rfx_inverse_mel_ex(None, None, 1, 1, 1, None, 0, None, None, 0, None, ctypes.byref(_start())) == -1 and b"takes no start" in lib.rfx_last_error()
    # a valid struct (start 0 or 1, with a loop too) passes the options and fails on the null plan
    for opt in (_start(), _start(start=0), _start(loop=1), _start(start=0, d_guide=0x1000, d_bins=0x3000)):
        assert _gl_ex(lib, opt) == -1 and b"null argument" in lib.rfx_last_error()
    # a loop-size caller (and the four shorter sizes) is unaffected by whatever lies behind its struct
    for size in (24, 48, 64, 80, 88):
        assert _gl_ex(lib, _start(start=2, reserved6=9, size=size)) == -1 and b"null argument" in lib.rfx_last_error(), size
    # flags == 2 stays refused: the start is not a flag bit
    assert _gl_ex(lib, _hip.RfxCallOptions(24, 2, 0, 0.0, 0.0)) == -1 and b"flags" in lib.rfx_last_error()
    # the queries answer 0 for a call with the start without a plan, like their drivers' own; the entry refuses a null plan and
    # takes B == 0 only with one
    assert helpers.need(lib, "griffinlim", None, 3, 41, start=1) == 0 == helpers.need(lib, "waveform_from_mel", None, 3, 41, start=1)
    assert helpers.need(lib, "audio_from_image", None, 3, 0, 41, start=1) == 0 == lib.rfx_peak_start_workspace_bytes(None, 3, 41)
    assert lib.rfx_peak_start(None, None, 0, 41, None, None, 0, None) == -1 and b"null argument" in lib.rfx_last_error()


def test_valid_options_size_nothing_without_a_plan(lib):
    """every served combination, and no options at all: 0 for a NULL plan, as the plain queries answer"""
    for fields in ({}, helpers.GUIDE, helpers.HELD, helpers.MASKED, dict(loop=1), dict(helpers.GUIDE, loop=1), dict(start=1), dict(loop=1, start=1),
                   dict(flags=1, loop=1, start=1, row_base=5, magnitude_hint=2.0)):
        assert helpers.need(lib, "waveform_from_mel", None, 3, 41, **fields) == 0 == helpers.need(lib, "audio_from_image", None, 3, 1, 41, **fields)
        if "flags" not in fields:
            assert helpers.need(lib, "griffinlim", None, 3, 41, **fields) == 0
    assert lib.rfx_griffinlim_workspace_bytes_ex(None, 3, 41, None) == 0 == lib.rfx_waveform_from_mel_workspace_bytes_ex(None, 3, 41, None)
    assert lib.rfx_audio_from_image_workspace_bytes_ex(None, 3, 1, 41, None) == 0 == lib.rfx_griffinlim_workspace_bytes(None, 3, 41)
    # Griffin-Lim itself reads no flag, as rfx_griffinlim_ex
    assert helpers.need(lib, "griffinlim", None, 3, 41, flags=1) == 0 and lib.rfx_last_error().startswith(b"rfx_griffinlim_workspace_bytes_ex: rfx_call_options.flags")


def test_cli_phase_start_flags(capsys):
    from riffusion import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--phase-start", "peaks", "--guide-audio", "g.wav"])
    assert e.value.code == 2 and "--phase-start peaks does not go with --guide-audio" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--phase-start peaks does not go with --guide-audio"):
        cli.image_to_audio(image="x.png", audio="y.wav", guide_audio="g.wav", phase_start="peaks")
    with pytest.raises(SystemExit) as e:
        cli.main(["image-to-audio", "--image", "x.png", "--audio", "y.wav", "--phase-start", "peak"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    parse = cli.build_parser().parse_args
    args = vars(parse(["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b", "--phase-start", "peaks", "--griffin-lim-iters", "4"]))
    assert (args["phase_start"], args["griffin_lim_iters"]) == ("peaks", 4)
    args = vars(parse(["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b"]))
    assert (args["phase_start"], args["griffin_lim_iters"]) == ("random", -1)
    assert vars(parse(["image-to-audio", "--image", "x.png", "--audio", "y.wav"]))["phase_start"] == "random"
    with pytest.raises(SystemExit) as e:
        cli.main(["images-to-audio-batch", "--image-dir", "a", "--output-dir", "b", "--griffin-lim-iters", "-3"])
    assert e.value.code == 2 and "--griffin-lim-iters must be >= 0" in capsys.readouterr().err


def test_python_layer_refuses_before_any_device_work():
    """phase_start="peaks" with another start or a hold, and any other string: ValueError from the converters without a device"""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramConverter.__new__(SpectrogramConverter)  # no device: the checks come first
    mel = torch.zeros(1, 512, 40)
    g = torch.zeros(1, 1000)
    for kw in (dict(guide=g), dict(angles0=torch.zeros(1, 8821, 40, dtype=torch.complex64)), dict(guide=g, hold_frames=(1, 1)),
               dict(guide=g, hold_mask=np.zeros((1, 512, 40), bool))):
        with pytest.raises(ValueError, match='phase_start="peaks" does not go with'):
            conv.waveform_from_mel_amplitudes(mel, phase_start="peaks", **kw)
    with pytest.raises(ValueError, match="phase_start must be one of"):
        conv.waveform_from_mel_amplitudes(mel, phase_start="beauregard")
    with pytest.raises(ValueError, match="phase_start must be one of"):
        conv.audio_from_spectrogram(np.zeros((1, 512, 40), np.float32), phase_start="")
    ic = SpectrogramImageConverter.__new__(SpectrogramImageConverter)
    ic.p = SpectrogramParams()
    tiles = np.zeros((1, 512, 40, 3), np.uint8)
    for fn in (ic.audio_from_spectrogram_images, ic.audio_from_spectrogram_image_sequence):
        with pytest.raises(ValueError, match='phase_start="peaks" does not go with guide_waveforms'):
            fn(tiles, phase_start="peaks", guide_waveforms=np.zeros((1, 1, 100), np.float32))
        with pytest.raises(ValueError, match="phase_start must be one of"):
            fn(tiles, phase_start="Peaks")
    with pytest.raises(ValueError, match='phase_start="peaks" does not go with guide_segment'):
        ic.audio_from_spectrogram_image(None, phase_start="peaks", guide_segment=object())
