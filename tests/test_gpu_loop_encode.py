"""
Loop forward calls on the device (include/rfx.h: rfx_stft_loop and the other *_loop forward entries): a row is one period of
P = hop T samples, frame t, element i reads x[(hop t + i - n_fft // 2) mod P]; the kernels are the plain forward kernels with the
sample position wrapped instead of reflected.

Parity is against tests/loop_oracle.py's loop_stft at the project's forward gates: complex spectrum relative max error below 2e-6
(test_stft_complex_matches_torch_stft), mel per-row max |diff| <= 1e-4 max(ref) and relative L2 <= 1e-4 (SURVEY 8(d),
test_mel_amplitudes_match_oracle).  The exact properties compare bytes.  Shapes: B = 3 rows of T = 41 frames on the four engines
(the smallest T all of them take, no multiple of 16), T = 40 on the specialised engine (period == n_fft: every frame wraps) and
B = 5, T = 120 there: 600 frames give a workgroup of the forward launch two frames (ceil(B T / (2 CUs)) on 256 CUs), so the wrap is
met inside a multi-frame walk and by the fused kernel's sliding prefetch.
"""
import os

import numpy as np
import pytest
import torch

import loop_oracle
from engines import CLIP2, ENGINES, bits as _bits, plan_for as _plan
from helpers import oracle, snr_db, synthetic_wave

pytestmark = pytest.mark.gpu

TILES = ["og_beat", "agile", "marim", "motorway", "vibes"]
SHAPES = [(name, 3, 41) for name in ENGINES] + [("specialised", 3, 40), ("specialised", 5, 120)]
SHAPE_IDS = [f"{name}-B{b}-T{t}" for name, b, t in SHAPES]
ALL = list(ENGINES)


@pytest.fixture(scope="module")
def O():
    return oracle()


_CASES = {}


def _case(O, name, B=3, frames=41):
    """(params, plan, op, x (B, P) on the host, x on the device, loop_stft(x) (B, n_stft, frames) complex64): computed once per engine
    and shape, never modified"""
    key = (name, B, frames)
    if key not in _CASES:
        p, plan = _plan(name)
        op = O.params_from(p)
        assert frames >= loop_oracle.min_frames(op)
        x = synthetic_wave(B, p.hop_length * frames, seed=101)
        ref = loop_oracle.loop_stft(O, x, op)
        assert ref.shape == (B, op.n_stft, frames)
        _CASES[key] = (p, plan, op, x, x.cuda(), ref)
    return _CASES[key]


def _thresholds(plan, p):
    from riffusion.util import image_util

    power = float(p.power_for_image)
    return plan.device_constant(("encode_thresholds", power), lambda: image_util.encode_thresholds(power))


# ---- parity with the oracle -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,frames", SHAPES, ids=SHAPE_IDS)
def test_spectrum_and_mel_match_the_oracle(O, name, B, frames):
    p, plan, op, x, xd, ref = _case(O, name, B, frames)
    if name == "specialised" and B * frames >= 600:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert -(-B * frames // (2 * cus)) >= 2, "this shape is here to give a workgroup more than one frame"
    assert plan.lib.rfx_stft_loop_frames(plan.handle, x.shape[1]) == frames
    mag, spec, Tn = plan.stft(xd, want_mag=True, want_spec=True, loop=True)
    assert Tn == frames
    got = plan.unpack_complex(spec, B, Tn).cpu()
    scale = ref.abs().max()
    err = float((got - ref).abs().max() / scale)
    l2 = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    print(f"loop stft {name} B={B} T={frames}: relative max error {err:.2e}, relative L2 {l2:.2e}")
    assert err < 2e-6 and l2 < 2e-6
    mag_from_spec = plan.pack_magnitudes(got.abs().cuda()).cpu()
    assert float((mag.cpu() - mag_from_spec).abs().max() / scale) < 1e-6  # padding positions are zero in both
    # mel: the oracle's MelScale of the oracle's circular magnitudes
    mel_ref = O.mel_scale(ref.abs(), O.mel_filterbank(op))
    mel = plan.mel_from_waveform(xd, loop=True).cpu()
    assert mel.shape == mel_ref.shape == (B, op.num_frequencies, frames)
    worst = max(float((mel[b] - mel_ref[b]).abs().max() / mel_ref[b].max()) for b in range(B))
    mel_l2 = float(torch.linalg.norm(mel - mel_ref) / torch.linalg.norm(mel_ref))
    print(f"loop mel {name} B={B} T={frames}: worst per-row max |diff| / max(ref) {worst:.2e}, relative L2 {mel_l2:.2e}")
    for b in range(B):
        assert (mel[b] - mel_ref[b]).abs().max() <= 1e-4 * mel_ref[b].max()
    assert mel_l2 <= 1e-4


# ---- exact properties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,frames", SHAPES, ids=SHAPE_IDS)
def test_rolled_input_gives_rolled_columns(O, name, B, frames):
    p, plan, op, x, xd, ref = _case(O, name, B, frames)
    thr = _thresholds(plan, p)
    mag, spec, _ = plan.stft(xd, want_mag=True, want_spec=True, loop=True)
    mel = plan.mel_from_waveform(xd, loop=True)
    img, mx = plan.image_from_waveform(xd, False, thr, loop=True)
    assert img.shape == (B, plan.n_mels, frames, 3) and float(mel.max()) > 0
    fs = plan.frame_stride
    for k in (1, 7, frames - 1):
        xr = torch.roll(xd, k * p.hop_length, dims=-1)
        mag_r, spec_r, _ = plan.stft(xr, want_mag=True, want_spec=True, loop=True)
        assert _bits(spec_r.reshape(B, frames, fs)) == _bits(torch.roll(spec.reshape(B, frames, fs), k, dims=1)), k
        assert _bits(mag_r.reshape(B, frames, fs)) == _bits(torch.roll(mag.reshape(B, frames, fs), k, dims=1)), k
        assert _bits(plan.mel_from_waveform(xr, loop=True)) == _bits(torch.roll(mel, k, dims=-1)), k
        img_r, mx_r = plan.image_from_waveform(xr, False, thr, loop=True)
        assert _bits(img_r) == _bits(torch.roll(img, k, dims=2)) and _bits(mx_r) == _bits(mx), k


@pytest.mark.parametrize("name,B,frames", SHAPES, ids=SHAPE_IDS)
def test_interior_columns_are_the_plain_entrys_bytes(O, name, B, frames):
    """x of P samples through the loop entry, x with one more sample through the unchanged plain entry (>= T frames): a frame whose
    window support [hop t + left - h, hop t + left + win - h) lies inside [0, P) reads the same samples in both, and must have the same
    bytes; the frames whose window reaches over an end read the wrapped signal in one and the reflected one in the other"""
    p, plan, op, x, xd, ref = _case(O, name, B, frames)
    P, hop = x.shape[1], op.hop_length
    x1 = torch.cat([xd, synthetic_wave(B, 1, seed=5).cuda()], dim=1).contiguous()
    lo = (op.n_fft - op.win_length) // 2 - op.n_fft // 2
    inside = [t for t in range(frames) if hop * t + lo >= 0 and hop * t + lo + op.win_length <= P]
    outside = [t for t in range(frames) if t not in inside]
    assert inside and outside and len(inside) + len(outside) == frames
    mag_l, spec_l, _ = plan.stft(xd, want_mag=True, want_spec=True, loop=True)
    mag_p, spec_p, T1 = plan.stft(x1, want_mag=True, want_spec=True)
    assert T1 >= frames
    mel_l, mel_p = plan.mel_from_waveform(xd, loop=True), plan.mel_from_waveform(x1)
    fs = plan.frame_stride
    views = {"spectrum": (spec_l.reshape(B, frames, fs), spec_p.reshape(B, T1, fs)), "magnitudes": (mag_l.reshape(B, frames, fs), mag_p.reshape(B, T1, fs)),
             "mel": (mel_l.transpose(1, 2), mel_p.transpose(1, 2))}
    for what, (a, b) in views.items():
        for t in inside:
            assert _bits(a[:, t]) == _bits(b[:, t]), (what, t)
        assert any(_bits(a[:, t]) != _bits(b[:, t]) for t in outside), what
    print(f"{name} T={frames}: {len(inside)} interior frames equal byte for byte, {len(outside)} frames reach over an end")


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_fused_image_entry_equals_its_parts(O, name, stereo):
    p, plan, op, x, xd, ref = _case(O, name, 4, 41)  # N = 4 mono clips, or N = 2 stereo ones
    thr = _thresholds(plan, p)
    img, mx = plan.image_from_waveform(xd, stereo, thr, loop=True)
    img2, mx2 = plan.image_encode(plan.mel_from_waveform(xd, loop=True), stereo, thr)
    assert img.shape == (2 if stereo else 4, plan.n_mels, 41, 3) and int(img.max()) > 0
    assert _bits(img) == _bits(img2) and _bits(mx) == _bits(mx2)
    lib = plan.lib
    N, Lw = img.shape[0], x.shape[1]
    parts = lib.rfx_mel_loop_workspace_bytes(plan.handle, 4, Lw)
    assert lib.rfx_image_from_waveform_loop_workspace_bytes(plan.handle, N, int(stereo), Lw) >= parts > 0


@pytest.mark.parametrize("name", ["specialised", "row-family-48k"])
def test_pcm16_clips_entry_equals_its_two_parts(O, name):
    p, plan, op, x, xd, ref = _case(O, name)
    thr = _thresholds(plan, p)
    P = x.shape[1]
    rng = np.random.default_rng(3)
    pcm = torch.from_numpy(rng.integers(-20000, 20000, size=(P + 3000, 2), dtype=np.int16)).cuda()
    starts = [0, 1234, 3000]
    for stereo in (False, True):
        C = 2 if stereo else 1
        img, mx = plan.image_from_pcm_clips(pcm, starts, P, stereo, thr, loop=True)
        wave = plan.clips_to_waveform(pcm, starts, P, C)
        img2, mx2 = plan.image_from_waveform(wave, stereo, thr, loop=True)
        assert img.shape == (3, plan.n_mels, 41, 3) and _bits(img) == _bits(img2) and _bits(mx) == _bits(mx2)
        # exactly the bytes of its parts: the gathered rows, then the fused image entry's workspace
        lib = plan.lib
        both = lib.rfx_image_from_pcm16_clips_loop_workspace_bytes(plan.handle, 3, int(stereo), P)
        fwd = lib.rfx_image_from_waveform_loop_workspace_bytes(plan.handle, 3, int(stereo), P)
        rows = -(-3 * C * P * 4 // 256) * 256
        assert both == rows + fwd


@pytest.mark.parametrize("name", ALL)
def test_a_row_has_the_same_bytes_alone(O, name):
    p, plan, op, x, xd, ref = _case(O, name)
    B, frames, fs = 3, 41, plan.frame_stride
    thr = _thresholds(plan, p)
    mag, spec, _ = plan.stft(xd, want_mag=True, want_spec=True, loop=True)
    mel = plan.mel_from_waveform(xd, loop=True)
    img, mx = plan.image_from_waveform(xd, False, thr, loop=True)
    for r in range(B):
        row = xd[r:r + 1].contiguous()
        mag_r, spec_r, _ = plan.stft(row, want_mag=True, want_spec=True, loop=True)
        assert _bits(spec_r) == _bits(spec.reshape(B, frames, fs)[r]) and _bits(mag_r) == _bits(mag.reshape(B, frames, fs)[r]), r
        assert _bits(plan.mel_from_waveform(row, loop=True)) == _bits(mel[r:r + 1]), r
        img_r, mx_r = plan.image_from_waveform(row, False, thr, loop=True)
        assert _bits(img_r) == _bits(img[r:r + 1]) and _bits(mx_r) == _bits(mx[r:r + 1]), r


# ---- closed loop: the analysis half of the loop decode ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specialised", "generic-11025"])
def test_stft_loop_of_a_loop_decode_is_the_guided_loop_start(O, name):
    """A loop decode y is a legal input of rfx_stft_loop and gives its T frames back.  A guided loop call with guide y at n_iter = 0
    analyses y inside the Griffin-Lim kernels, projects - Z = S G / (|G| + 1e-16) - and synthesises; the same projection of the
    spectrum rfx_stft_loop gives for y, synthesised by the oracle in float64, must be that audio.  By the parity rule of
    test_guided_loop_start_is_the_phase_of_the_circular_stft: against the float64 oracle's result, no more than 6 dB below the
    float32 oracle's SNR: that is the gate, for the guided start and for rfx_stft_loop's direction.  One check on top of it, no gate of
    the issue's: the two device analyses then agree with each other to within the sum of their two errors, 12 dB below."""
    p, plan, op, x, xd, ref = _case(O, name)
    B, frames = 3, 41
    mag = ref.abs()
    S = plan.pack_magnitudes(mag.cuda())
    a0 = torch.rand(mag.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(7))
    y = plan.griffinlim(S, B, frames, 2, 0.99, angles0_slots=plan.pack_complex(a0.cuda()), loop=True)
    assert y.shape == (B, plan.output_samples(frames, True)) and plan.lib.rfx_stft_loop_frames(plan.handle, y.shape[1]) == frames
    _, spec, Tn = plan.stft(y, want_mag=False, want_spec=True, loop=True)
    G = plan.unpack_complex(spec, B, Tn).cpu()
    yh = y.cpu()
    G32, G64 = loop_oracle.loop_stft(O, yh, op), loop_oracle.loop_stft(O, yh, op, torch.float64)
    err = float((G - G32).abs().max() / G32.abs().max())
    assert Tn == frames and err < 2e-6
    want32 = loop_oracle.loop_istft(O, mag * (G32 / (G32.abs() + 1e-16)), op, torch.float32)
    want64 = loop_oracle.loop_istft(O, mag.double() * (G64 / (G64.abs() + 1e-16)), op, torch.float64)
    Gd = G.to(torch.complex128)
    from_entry = loop_oracle.loop_istft(O, mag.double() * (Gd / (Gd.abs() + 1e-16)), op, torch.float64)
    guided = plan.griffinlim(S, B, frames, 0, 0.99, guide=y, loop=True).cpu()
    o32, dev, ent, both = snr_db(want64, want32), snr_db(want64, guided), snr_db(want64, from_entry), snr_db(guided, from_entry)
    print(f"{name}: float32 oracle vs float64 oracle {o32:.1f} dB; guided start (n_iter 0) vs float64 oracle {dev:.1f} dB; rfx_stft_loop's direction, "
          f"synthesised in float64, vs float64 oracle {ent:.1f} dB; the two against each other {both:.1f} dB")
    assert dev >= o32 - 6.0 and ent >= o32 - 6.0 and both >= o32 - 12.0


# ---- rfx_spectral_error_loop -------------------------------------------------------------------------------------------------------------

def _golden_rgb(golden_dir, name):
    from PIL import Image

    from riffusion.util import image_util

    with Image.open(os.path.join(golden_dir, f"{name}.png")) as im:
        return np.ascontiguousarray(np.asarray(image_util.rgb_array_from_image(im)))


def test_circular_spectral_convergence_against_the_oracle(O, golden_dir):
    """4-iteration loop decodes of columns [100:164] of the five golden tiles, by the rule of
    test_spectral_convergence_against_the_oracle: the float32 oracle's own distance from its float64 figure (loop_stft and both norms
    in float32, against loop_oracle.loop_spectral_convergence) is measured on the same inputs in the same run, and twice the largest
    is allowed - against the float32 figure as there, and against the float64 figure."""
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    params = SpectrogramParams(num_griffin_lim_iters=4)
    op = O.params_from(params)
    conv = SpectrogramConverter(params, device="cuda")
    plan = conv._plan()
    n, T = len(TILES), 64
    mel = torch.from_numpy(np.concatenate([O.spectrogram_from_image_u8(_golden_rgb(golden_dir, t)[:, 100:100 + T], 0.25, False, 30e6) for t in TILES]))
    lin_slots = plan.inverse_mel(mel.cuda(), 1, seed=3)
    wave = plan.griffinlim(lin_slots, n, T, 4, 0.99, seed=4, loop=True)
    assert wave.shape == (n, op.hop_length * T)
    lin = plan.unpack_magnitudes(lin_slots, n, T)
    got = conv.spectral_convergence(wave, lin, loop=True)
    assert got.shape == (n,) and got.dtype == torch.float64
    sums = plan.spectral_error(wave, lin_slots, n, T, loop=True)
    assert _bits(got) == _bits(conv.convergence_from_sums(*sums.unbind(1)))
    assert _bits(got) != _bits(conv.spectral_convergence(wave[:, :op.hop_length * (T - 1)].contiguous(), lin))  # (the reflect-padded figure of the cut clip is another)
    wave_h, lin_h = wave.cpu(), lin.cpu()
    want32, want64 = [], []
    for i in range(n):
        want64.append(loop_oracle.loop_spectral_convergence(O, wave_h[i:i + 1], lin_h[i:i + 1], op))
        S = lin_h[i:i + 1]
        want32.append(float((loop_oracle.loop_stft(O, wave_h[i:i + 1], op, torch.float32).abs() - S).norm() / S.norm()))
    oracle_distance = max(abs(a - b) / b for a, b in zip(want32, want64))
    rel32 = [abs(float(got[i]) - want32[i]) / want32[i] for i in range(n)]
    rel64 = [abs(float(got[i]) - want64[i]) / want64[i] for i in range(n)]
    for i, tile in enumerate(TILES):
        print(f"{tile}: device {float(got[i]):.9f}, oracle float32 {want32[i]:.9f}, float64 {want64[i]:.9f}; device vs float32 oracle {rel32[i]:.2e}, "
              f"oracle float32 vs float64 {abs(want32[i] - want64[i]) / want64[i]:.2e}, device vs float64 {rel64[i]:.2e}")
    print(f"oracle's largest float32-vs-float64 distance on these inputs {oracle_distance:.2e}, bound 2 x that")
    assert oracle_distance > 0 and max(rel32) <= 2.0 * oracle_distance and max(rel64) <= 2.0 * oracle_distance
    # a row's two sums are the same bytes alone and inside the batch
    row_elems = T * plan.frame_stride
    for r in (0, 3):
        alone = plan.spectral_error(wave[r:r + 1].contiguous(), lin_slots.reshape(-1)[r * row_elems:(r + 1) * row_elems].contiguous(), 1, T, loop=True)
        assert _bits(alone) == _bits(sums[r:r + 1]), r
    # the bounded workspace of the plain entry
    assert plan.lib.rfx_spectral_error_loop_workspace_bytes(plan.handle, n, T) == plan.lib.rfx_spectral_error_workspace_bytes(plan.handle, n, T) > 0


def test_return_loop_error_leaves_the_pcm_bytes_unchanged(golden_dir):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False, num_griffin_lim_iters=4), device="cuda")
    tiles = np.stack([_golden_rgb(golden_dir, t)[:, 100:164] for t in TILES[:3]])
    pcm = conv.audio_from_spectrogram_images(tiles, loop=True, seed=21)
    pcm_e, err = conv.audio_from_spectrogram_images(tiles, loop=True, seed=21, return_loop_error=True)
    assert pcm.shape == (3, conv.p.hop_length * 64, 1) and np.array_equal(pcm, pcm_e)
    assert isinstance(err, np.ndarray) and err.shape == (3,) and err.dtype == np.float64 and np.isfinite(err).all() and (err > 0).all() and (err < 1).all()
    pcm_1, err_1 = conv.audio_from_spectrogram_images(tiles, loop=True, seed=21, return_loop_error=True, tiles_per_call=1)
    assert np.array_equal(pcm_1, pcm) and np.array_equal(err_1, err)
    print("circular spectral convergence of 4-iteration loop decodes:", np.round(err, 4).tolist())
    with pytest.raises(ValueError, match="it needs loop=True"):
        conv.audio_from_spectrogram_images(tiles, seed=21, return_loop_error=True)
    with pytest.raises(ValueError, match="return_error"):
        conv.audio_from_spectrogram_images(tiles, loop=True, return_error=True)


# ---- refusals launch nothing --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specialised", "generic-11025"])
def test_refusals_launch_nothing(O, name):
    """every refusal comes before any launch and leaves the output buffers as they were (canary-filled)"""
    from riffusion import _hip

    p, plan, op, x, xd, ref = _case(O, name)
    lib, h = plan.lib, plan.handle
    B, frames, P, hop = 3, 41, x.shape[1], op.hop_length
    fs, M = plan.frame_stride, plan.n_mels
    stream = _hip.current_stream(torch.device("cuda"))
    thr = _thresholds(plan, p)
    long = torch.cat([xd, xd], dim=1).contiguous()  # rows long enough for every length tried below
    mag = torch.full((B * (frames + 1), fs), 123.0, device="cuda")
    spec = torch.full((B * (frames + 1), fs, 2), 123.0, device="cuda")
    mel = torch.full((B, M, frames + 1), 123.0, device="cuda")
    img = torch.full((B, M, frames + 1, 3), 77, dtype=torch.uint8, device="cuda")
    mx = torch.full((B,), 123.0, device="cuda")
    sums = torch.full((B, 2), 123.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(lib.rfx_image_from_pcm16_clips_loop_workspace_bytes(h, B, 0, P + hop), lib.rfx_spectral_error_loop_workspace_bytes(h, B, frames)) + 4096,
                     dtype=torch.uint8, device="cuda")
    pcm = torch.zeros((2 * P, 1), dtype=torch.int16, device="cuda")
    starts_h = torch.tensor([0, 5, 9], dtype=torch.int64)
    starts_d = starts_h.cuda()

    def untouched():
        torch.cuda.synchronize()
        return (bool((mag == 123.0).all()) and bool((spec == 123.0).all()) and bool((mel == 123.0).all()) and bool((img == 77).all())
                and bool((mx == 123.0).all()) and bool((sums == 123.0).all()))

    low = hop * loop_oracle.min_frames(op)
    for Lw in (P - 1, P + 1, low - hop, 0, -1):
        assert lib.rfx_stft_loop_frames(h, Lw) == 0 == lib.rfx_mel_loop_workspace_bytes(h, B, Lw)
        assert lib.rfx_image_from_waveform_loop_workspace_bytes(h, B, 0, Lw) == 0 == lib.rfx_image_from_pcm16_clips_loop_workspace_bytes(h, B, 0, Lw)
        calls = {
            "rfx_stft_loop": lambda: lib.rfx_stft_loop(h, long.data_ptr(), B, Lw, mag.data_ptr(), spec.data_ptr(), stream),
            "rfx_mel_from_waveform_loop": lambda: lib.rfx_mel_from_waveform_loop(h, long.data_ptr(), B, Lw, mel.data_ptr(), ws.data_ptr(), ws.numel(), stream),
            "rfx_image_from_waveform_loop": lambda: lib.rfx_image_from_waveform_loop(h, long.data_ptr(), B, 0, Lw, thr.data_ptr(), mx.data_ptr(), img.data_ptr(),
                                                                                     ws.data_ptr(), ws.numel(), stream),
        }
        if Lw > 0:  # (a clip of no frames is refused by the clip checks the plain entry has, before the length rule)
            calls["rfx_image_from_pcm16_clips_loop"] = lambda: lib.rfx_image_from_pcm16_clips_loop(
                h, pcm.data_ptr(), 2 * P, 1, starts_h.data_ptr(), starts_d.data_ptr(), B, Lw, 0, thr.data_ptr(), mx.data_ptr(), img.data_ptr(), ws.data_ptr(),
                ws.numel(), stream)
        for who, call in calls.items():
            assert call() == -1, (who, Lw)
            why = lib.rfx_last_error().decode()
            assert who + ":" in why and "nearest legal lengths" in why and f"got {Lw}:" in why, why
            assert untouched(), (who, Lw)
    # the spectral error of a loop decode of too few frames
    T_bad = loop_oracle.min_frames(op) - 1
    assert lib.rfx_spectral_error_loop_workspace_bytes(h, B, T_bad) == 0
    assert lib.rfx_spectral_error_loop(h, long.data_ptr(), mag.data_ptr(), B, T_bad, sums.data_ptr(), ws.data_ptr(), ws.numel(), stream) == -1
    assert b"rfx_spectral_error_loop" in lib.rfx_last_error() and untouched()
    # a workspace one byte short
    short = [
        (lib.rfx_mel_loop_workspace_bytes(h, B, P),
         lambda n: lib.rfx_mel_from_waveform_loop(h, xd.data_ptr(), B, P, mel.data_ptr(), ws.data_ptr(), n, stream)),
        (lib.rfx_image_from_waveform_loop_workspace_bytes(h, B, 0, P),
         lambda n: lib.rfx_image_from_waveform_loop(h, xd.data_ptr(), B, 0, P, thr.data_ptr(), mx.data_ptr(), img.data_ptr(), ws.data_ptr(), n, stream)),
        (lib.rfx_image_from_pcm16_clips_loop_workspace_bytes(h, B, 0, P),
         lambda n: lib.rfx_image_from_pcm16_clips_loop(h, pcm.data_ptr(), 2 * P, 1, starts_h.data_ptr(), starts_d.data_ptr(), B, P, 0, thr.data_ptr(),
                                                       mx.data_ptr(), img.data_ptr(), ws.data_ptr(), n, stream)),
        (lib.rfx_spectral_error_loop_workspace_bytes(h, B, frames),
         lambda n: lib.rfx_spectral_error_loop(h, xd.data_ptr(), mag.data_ptr(), B, frames, sums.data_ptr(), ws.data_ptr(), n, stream)),
    ]
    for need, call in short:
        assert need > 0 and call(need - 1) == -3, lib.rfx_last_error()
        assert b"workspace too small" in lib.rfx_last_error() and untouched()
    # the Python layer refuses before any device work as well
    with pytest.raises(ValueError, match="nearest legal lengths"):
        plan.stft(long[:, :P + 1].contiguous(), True, True, loop=True)
    with pytest.raises(ValueError, match="nearest legal lengths"):
        plan.mel_from_waveform(long[:, :P - 1].contiguous(), loop=True)
    with pytest.raises(ValueError, match="nearest legal lengths"):
        plan.image_from_waveform(long[:, :P + 1].contiguous(), False, thr, loop=True)
    with pytest.raises(ValueError, match="nearest legal lengths"):
        plan.image_from_pcm_clips(pcm, [0], P + 1, False, thr, loop=True)
    with pytest.raises(ValueError, match="at least"):
        plan.spectral_error(long[:, :hop * T_bad].contiguous(), mag, B, T_bad, loop=True)


# ---- the product entry points and the CLI ---------------------------------------------------------------------------------------------------

def _cut_clip(golden_dir, tmp_path):
    """golden clip 2 cut to its first 512 hops: (segment, path of the cut file, path of the uncut file)"""
    from riffusion.util import audio_util

    src = os.path.join(golden_dir, CLIP2 + ".wav")
    whole = audio_util.PcmSegment.from_wav(src)
    P = 512 * 441
    assert whole.frame_rate == 44100 and int(whole.frame_count()) > P
    cut = audio_util.PcmSegment(np.asarray(whole.get_array_of_samples()).reshape(-1, whole.channels)[:P].copy(), whole.frame_rate)
    path = str(tmp_path / "loop_clip.wav")
    cut.export(path, format="wav")
    return cut, path, src


def test_product_loop_encode_and_the_cli(golden_dir, tmp_path, capsys):
    from PIL import Image

    from riffusion import cli
    from riffusion.spectrogram_converter import LoopLengthError
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    cut, cut_path, whole_path = _cut_clip(golden_dir, tmp_path)
    params = SpectrogramParams(sample_rate=44100, stereo=False)
    conv = SpectrogramImageConverter(params, device="cuda")
    image = conv.spectrogram_image_from_audio(cut, loop=True)
    assert image.size == (512, 512)
    assert SpectrogramParams.from_exif(image.getexif()) == params  # the EXIF round-trips ...
    max_value = float(image.getexif()[SpectrogramParams.ExifTags.MAX_VALUE.value])
    # ... and the image bytes are the fused C entry's
    plan = conv.converter._plan()
    mono = cut.set_channels(1)
    wave = torch.from_numpy(np.asarray(mono.get_array_of_samples(), dtype=np.float32)[None]).cuda()
    img, mx = plan.image_from_waveform(wave, False, _thresholds(plan, params), loop=True)
    assert np.array_equal(np.asarray(image), img[0].cpu().numpy()) and max_value == float(mx[0])
    plain = conv.spectrogram_image_from_audio(cut)
    assert plain.size == (513, 512) and not np.array_equal(np.asarray(plain)[:, :512], np.asarray(image))
    # the mel tensor and the clips entry take the keyword too
    mel = conv.converter.spectrogram_from_audio(mono, loop=True)
    assert mel.shape == (1, 512, 512) and np.array_equal(mel, plan.mel_from_waveform(wave, loop=True).cpu().numpy())
    images, _ = conv.spectrogram_images_from_audio_clips(cut, [0.0], 5.12, loop=True)
    assert np.array_equal(np.asarray(images[0]), np.asarray(image))
    files, _ = conv.spectrogram_images_from_waveforms(wave[None].cpu(), as_png=True, loop=True)
    import io

    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB")), np.asarray(image))
    # the CLI writes the same tile
    out = str(tmp_path / "loop.png")
    cli.main(["audio-to-image", "--audio", cut_path, "--image", out, "--loop"])
    with Image.open(out) as written:
        assert written.size == (512, 512) and np.array_equal(np.asarray(written.convert("RGB")), np.asarray(image))
        assert SpectrogramParams.from_exif(written.getexif()) == params
    # ... and refuses the uncut file with the length message
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(["audio-to-image", "--audio", whole_path, "--image", str(tmp_path / "no.png"), "--loop"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "nearest legal lengths" in err and "250047 samples (5670.000 ms) below" in err and "250488 samples (5680.000 ms) above" in err
    assert not os.path.exists(str(tmp_path / "no.png"))
    whole = audio_util.PcmSegment.from_wav(whole_path)
    with pytest.raises(LoopLengthError):
        conv.spectrogram_image_from_audio(whole, loop=True)
    with pytest.raises(LoopLengthError):  # 5003 ms are 220632 frames: 500.3 hops
        conv.spectrogram_images_from_audio_clips(whole, [0.0], 5.003, loop=True)
    with pytest.raises(ValueError, match="reaches past the track's end"):
        conv.spectrogram_images_from_audio_clips(whole, [1.0], 5.0, loop=True)
    # image-to-audio --loop --print-error decodes the tile to the clip's length and prints the circular figure
    wav = str(tmp_path / "back.wav")
    torch.manual_seed(5)
    cli.main(["image-to-audio", "--image", out, "--audio", wav, "--loop", "--print-error", "--griffin-lim-iters", "4"])
    printed = capsys.readouterr().out
    assert "Spectral convergence (circular STFT): 0." in printed
    torch.manual_seed(5)
    segment, error = conv.audio_from_spectrogram_image(Image.open(out), griffin_lim_iters=4, loop=True, return_loop_error=True)
    assert f"Spectral convergence (circular STFT): {error:.6f}" in printed
    assert np.array_equal(np.asarray(segment.get_array_of_samples()), np.asarray(audio_util.PcmSegment.from_wav(wav).get_array_of_samples()))
    with pytest.raises(ValueError, match="it needs loop=True"):
        conv.audio_from_spectrogram_image(Image.open(out), return_loop_error=True)
    assert int(audio_util.PcmSegment.from_wav(wav).frame_count()) == 512 * 441
