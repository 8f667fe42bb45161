"""
Batches at the sizes where launch geometry and index arithmetic go wrong: more than 65535 rows in one call (a batch put on a
grid dimension that is only 16 bits wide on some runtimes) and slot arrays past 2^31 elements / 4 GiB of byte offset.

Every assertion is bit equality, against either a plain host / torch reference of the same operation (the slot permutation, the
image codec, PCM, filters and stitching) or the same rows computed alone: a clip's output depends only on the clip, the seed and
its global row (rfx_call_options.row_base), so a row at the far end of a giant batch has an exact reference in a one-row call.
Rows are checked on both sides of each boundary: 0, 65534, 65535, 65536 and the last; for the offsets 222 / 223 / 224 (4 GiB of
float slots), 445 / 446 / 447 (2^31 float elements) and the last.  Each case frees its buffers before the next one.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID_ROWS = 65536 + 7
GRID_CHECK = (0, 1, 65534, 65535, 65536, GRID_ROWS - 1)
OFFSET_TILES = 448
OFFSET_CHECK = (0, 222, 223, 224, 445, 446, 447)
GIB = 1 << 30


def _require(gib: float) -> None:
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib:.0f} GiB of free device memory, {free / GIB:.1f} GiB free")


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    from riffusion import _hip

    gc.collect()
    if not torch.cuda.is_available():
        return
    with _hip._plans_lock:
        plans = list(_hip._plans.values())
    for plan in plans:
        plan.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _params(**kw):
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramParams(**kw)


def _plan(**kw):
    from riffusion import _hip

    opts = {k: kw.pop(k) for k in ("gl_form", "frame_engine", "plan_layout") if k in kw}
    return _hip.get_plan(_params(**kw), "cuda:0", **opts)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cuda").manual_seed(seed)


def _bits(t: torch.Tensor) -> torch.Tensor:
    """Bit pattern of a float / complex tensor, so that equality is bit equality (signed zeros, NaN payloads)."""
    t = t.contiguous()
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int32)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ---- the specialised engine's slot layout (csrc/rfx_core.h), written out in numpy -------------------------------------------
N_FFT, N_BINS, Q_PAD, FRAME_STRIDE = 17640, 8821, 448, 9408


def _slot_maps(complex_: bool):
    """(pos_bin, pos_conj, bin_pos): the bin each slot position holds (-1: padding) and whether it holds its conjugate, and the
    primary position of every bin (the one the unpack reads)."""
    per = 2 if complex_ else 4
    pos_bin = np.full(FRAME_STRIDE, -1, np.int64)
    pos_conj = np.zeros(FRAME_STRIDE, bool)
    for p in range(FRAME_STRIDE):
        if p < 20 * Q_PAD:
            g, rem = divmod(p, per * Q_PAD)
            qp, kb = rem // per, per * g + rem % per
        else:
            qp, kb = p - 20 * Q_PAD, 20
        if qp % 64 == 63:
            continue
        q = (qp // 64) * 63 + qp % 64
        k = q // 21 + 40 * (q % 21 + 21 * kb)
        pos_conj[p] = k > N_FFT // 2
        pos_bin[p] = N_FFT - k if pos_conj[p] else k

    def pos_of(q, kb):
        qp = q + q // 63
        return ((kb // per) * Q_PAD + qp) * per + kb % per if kb < 20 else 20 * Q_PAD + qp

    bin_pos = np.empty(N_BINS, np.int64)
    for b in range(N_BINS):
        k = N_FFT - b if b % 40 > 20 else b
        kp = k // 40
        bin_pos[b] = pos_of((k % 40) * 21 + kp % 21, kp // 21)
    return pos_bin, pos_conj, bin_pos


def test_slot_maps_are_a_layout():
    """The numpy maps above describe a layout: every bin is held, its primary slot holds it, padding is 63 lanes of 64."""
    for complex_ in (False, True):
        pos_bin, pos_conj, bin_pos = _slot_maps(complex_)
        assert set(pos_bin[pos_bin >= 0].tolist()) == set(range(N_BINS))
        assert np.array_equal(pos_bin[bin_pos], np.arange(N_BINS))
        assert int((pos_bin < 0).sum()) == 21 * 7
        assert int(pos_conj.sum()) > 0


def _pack_reference(bft_clip: torch.Tensor, complex_: bool) -> torch.Tensor:
    """(F, T) -> (T, stride): slot p of frame t holds bin pos_bin[p] of frame t, conjugated on a conjugate slot, zero on padding."""
    pos_bin, pos_conj, _ = _slot_maps(complex_)
    idx = torch.from_numpy(np.maximum(pos_bin, 0)).to(bft_clip.device)
    rows = bft_clip[idx].transpose(0, 1)
    if complex_:
        rows = torch.where(torch.from_numpy(pos_conj).to(bft_clip.device), rows.conj().resolve_conj(), rows)
    return torch.where(torch.from_numpy(pos_bin >= 0).to(bft_clip.device), rows, torch.zeros((), dtype=rows.dtype, device=rows.device))


def _unpack_reference(slot_rows: torch.Tensor, complex_: bool) -> torch.Tensor:
    """(T, stride) -> (F, T): every bin read from its primary slot, conjugated where that slot holds the conjugate."""
    pos_bin, pos_conj, bin_pos = _slot_maps(complex_)
    out = slot_rows[:, torch.from_numpy(bin_pos).to(slot_rows.device)].transpose(0, 1)
    if complex_:
        conj = torch.from_numpy(pos_conj[bin_pos]).to(slot_rows.device)[:, None]
        out = torch.where(conj, out.conj().resolve_conj(), out)
    return out


# ---- A: more than 65535 rows in one call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("complex_", [False, True], ids=["float", "complex"])
def test_specialised_pack_unpack_past_65535_clips(complex_):
    """pack_kernel / unpack_mag_kernel / unpack_complex_kernel put the clip on grid z: 65 543 clips of T = 2 frames (one partial
    16-frame chunk).  The slots of the boundary clips equal the numpy permutation of rfx_core.h, and the round trip is exact
    for the whole batch (a dropped clip would leave zeros in the slots and garbage in the unpacked tensor)."""
    _require(32 if complex_ else 16)
    plan = _plan()
    B, T = GRID_ROWS, 2
    dtype = torch.complex64 if complex_ else torch.float32
    bft = torch.randn((B, plan.n_stft, T), dtype=dtype, device="cuda", generator=_gen(1))
    slots = plan.pack_complex(bft) if complex_ else plan.pack_magnitudes(bft)
    for c in GRID_CHECK:
        assert _same(slots[c * T:(c + 1) * T], _pack_reference(bft[c], complex_)), f"pack: clip {c}"
    back = plan.unpack_complex(slots, B, T) if complex_ else plan.unpack_magnitudes(slots, B, T)
    for c in GRID_CHECK:
        assert _same(back[c], _unpack_reference(slots[c * T:(c + 1) * T], complex_)), f"unpack: clip {c}"
    assert _same(back, bft), "pack + unpack is not the identity on every clip"


@pytest.mark.parametrize("rate,engine", [(11025, "generic"), (48000, "generic")])
def test_generic_pack_unpack_past_65535_clips(rate, engine):
    """gen_pack_kernel / gen_unpack_kernel (clip on grid z): plain bin-ordered frames, zero beyond n_stft, at 65 543 clips."""
    _require(12)
    plan = _plan(sample_rate=rate, frame_engine=engine)
    assert plan.generic
    B, T, F = GRID_ROWS, 3, plan.n_stft
    for dtype in (torch.float32, torch.complex64):
        bft = torch.randn((B, F, T), dtype=dtype, device="cuda", generator=_gen(rate))
        slots = plan.pack_complex(bft) if dtype.is_complex else plan.pack_magnitudes(bft)
        for c in GRID_CHECK:
            want = torch.zeros((T, plan.frame_stride), dtype=dtype, device="cuda")
            want[:, :F] = bft[c].transpose(0, 1)
            assert _same(slots[c * T:(c + 1) * T], want), (dtype, c)
        back = plan.unpack_complex(slots, B, T) if dtype.is_complex else plan.unpack_magnitudes(slots, B, T)
        assert _same(back, bft), dtype
        del bft, slots, back


def _mel_batch(plan, B, T, seed):
    g = _gen(seed)
    return torch.rand((B, plan.n_mels, T), device="cuda", generator=g) * 3e6


def _rows_alone_equal(whole, one_row, rows):
    for r in rows:
        alone = one_row(r)
        assert _same(whole[r:r + 1], alone), f"row {r}: {int((whole[r:r + 1] != alone).sum())} samples differ from the row alone"


def _require_workspace(plan, B, T, extra_gib=0.0):
    _require(plan.lib.rfx_waveform_from_mel_workspace_bytes(plan.handle, B, T) / GIB + extra_gib + 2)


# Griffin-Lim iterations need at least 22 frames (the inverse STFT's reflect padding, as in the reference): at 65 536 rows of the
# specialised engine that is 54 GB of magnitude slots alone, so the specialised cases run the initial inverse STFT (n_iter = 0),
# which launches the same fold and range pass; the generic engine at 11.025 kHz runs an iteration too.
@pytest.mark.parametrize("gl_form", ["runs", "frames"])
@pytest.mark.parametrize("T", [2, 4])
def test_specialised_waveform_from_mel_past_65535_rows(gl_form, T):
    """InverseMelScale + Griffin-Lim of 65 543 one-channel clips in one call (gl_fold_kernel: row on grid y in the per-frame form;
    the range pass from the data, magnitude_hint = 0, over 65 543 clips) equals each boundary row converted alone at its row_base."""
    n_iter = 0
    plan = _plan(gl_form=gl_form)
    _require_workspace(plan, GRID_ROWS, T, 1)
    mel = _mel_batch(plan, GRID_ROWS, T, seed=T)
    whole = plan.waveform_from_mel(mel, 1, n_iter, seed=9)
    assert whole.shape == (GRID_ROWS, plan.hop_length * (T - 1))
    _rows_alone_equal(whole, lambda r: plan.waveform_from_mel(mel[r:r + 1], 1, n_iter, seed=9, row_base=r), GRID_CHECK)
    # stereo clips: the range pass groups two rows per clip, the fold still has one row per grid y
    whole2 = plan.waveform_from_mel(mel[:GRID_ROWS - 1], 2, n_iter, seed=9)
    for r in (0, 65534, 65536, GRID_ROWS - 3):
        alone = plan.waveform_from_mel(mel[r:r + 2], 2, n_iter, seed=9, row_base=r)
        assert _same(whole2[r:r + 2], alone), f"stereo rows {r}, {r + 1}"


@pytest.mark.parametrize("gl_form", ["runs", "frames"])
def test_specialised_griffinlim_past_65535_rows(gl_form):
    """rfx_griffinlim on slots with the range pass over 65 543 rows (magnitude_hint = 0) and then with a hint."""
    _require(32)
    plan = _plan(gl_form=gl_form)
    B, T, n_iter = GRID_ROWS, 2, 0
    mag = plan.pack_magnitudes(torch.rand((B, plan.n_stft, T), device="cuda", generator=_gen(3)) * 1000.0)
    for hint in (0.0, 1000.0):
        whole = plan.griffinlim(mag, B, T, n_iter, seed=5, magnitude_hint=hint)
        _rows_alone_equal(whole, lambda r: plan.griffinlim(mag[r * T:(r + 1) * T], 1, T, n_iter, seed=5, row_base=r, magnitude_hint=hint),
                          GRID_CHECK)
        del whole


@pytest.mark.parametrize("rate,engine,T,iters", [(11025, "auto", 22, (0, 1)), (22050, "generic", 3, (0,)), (48000, "auto", 3, (0,))])
def test_other_engines_waveform_from_mel_past_65535_rows(rate, engine, T, iters):
    """The generic engine (11.025 kHz; 22.05 kHz forced onto it) with gen_fold / gen_fold4 (row on grid y), and the row-family
    engine at 48 kHz: 65 543 rows in one call equal the boundary rows alone."""
    plan = _plan(sample_rate=rate, frame_engine=engine)
    assert plan.griffinlim_engine == ("row-family" if rate == 48000 else "generic")
    _require_workspace(plan, GRID_ROWS, T, 1)
    mel = _mel_batch(plan, GRID_ROWS, T, seed=rate)
    for n_iter in iters:
        whole = plan.waveform_from_mel(mel, 1, n_iter, seed=2)
        _rows_alone_equal(whole, lambda r: plan.waveform_from_mel(mel[r:r + 1], 1, n_iter, seed=2, row_base=r), GRID_CHECK)


def _host_image(mel_clip: np.ndarray) -> np.ndarray:
    from riffusion.util import image_util

    return np.asarray(image_util.image_from_spectrogram(mel_clip))


@pytest.mark.parametrize("stereo", [False, True])
def test_forward_past_65535_clips(stereo):
    """image_from_waveform (stft_mel + image_encode_tm_kernel: image on grid z) and mel_from_waveform (mel_transpose_kernel: row on
    grid z) of 65 543 clips of n_fft / 2 + 1 samples: the boundary clips equal the same clips alone, and their images equal the
    host quantisation of the device mel."""
    from riffusion.util import image_util

    _require(24)
    plan = _plan()
    C = 2 if stereo else 1
    N, Lw = GRID_ROWS, plan.n_fft // 2 + 1
    wave = torch.randn((N * C, Lw), device="cuda", generator=_gen(8)) * 8000.0
    thr = plan.device_constant(("encode_thresholds", 0.25), lambda: image_util.encode_thresholds(0.25))
    img, mx = plan.image_from_waveform(wave, stereo, thr)
    mel = plan.mel_from_waveform(wave)
    T = plan.lib.rfx_stft_frames(plan.handle, Lw)
    assert img.shape == (N, plan.n_mels, T, 3) and mel.shape == (N * C, plan.n_mels, T)
    for n in GRID_CHECK:
        rows = wave[n * C:(n + 1) * C]
        img1, mx1 = plan.image_from_waveform(rows, stereo, thr)
        assert torch.equal(img[n:n + 1], img1) and _same(mx[n:n + 1], mx1), f"image of clip {n}"
        mel_n = mel[n * C:(n + 1) * C]
        assert _same(mel_n, plan.mel_from_waveform(rows)), f"mel of clip {n}"
        host = mel_n.cpu().numpy()
        assert float(mx[n]) == float(host.max())
        assert np.array_equal(img[n].cpu().numpy(), _host_image(host)), f"image of clip {n} vs the host quantisation"


@pytest.mark.parametrize("stereo", [False, True])
def test_image_codec_past_65535_clips(stereo):
    """image_encode_kernel (image on grid z) and image_decode_kernel at 65 543 images of T = 3 columns against the host codec.
    The decode's one-workgroup-per-row grid is 2^32 work-items long at 32 768 images of 512 rows: it is launched in pieces."""
    from riffusion.util import image_util

    _require(8)
    plan = _plan()
    C = 2 if stereo else 1
    N, T = GRID_ROWS, 3
    mel = torch.rand((N * C, plan.n_mels, T), device="cuda", generator=_gen(12)) ** 4 * 3e6
    thr = plan.device_constant(("encode_thresholds", 0.25), lambda: image_util.encode_thresholds(0.25))
    img, mx = plan.image_encode(mel, stereo, thr)
    lut_host = image_util.decode_lut(0.25, 30e6)
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: lut_host)
    dec = plan.image_decode(img, stereo, lut)
    planes = [1, 2] if stereo else [0]
    for n in GRID_CHECK:
        host = mel[n * C:(n + 1) * C].cpu().numpy()
        assert float(mx[n]) == float(host.max()), f"max of clip {n}"
        got = img[n].cpu().numpy()
        assert np.array_equal(got, _host_image(host)), f"image of clip {n}"
        want = lut_host[got[::-1][:, :, planes].transpose(2, 0, 1)]
        assert np.array_equal(dec[n * C:(n + 1) * C].cpu().numpy().view(np.int32), want.view(np.int32)), f"decode of clip {n}"


def _pcm_batch(N, L, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 3000, (N, L, C)).astype(np.int16)
    x[1::5] //= 64  # quiet clips: large gains
    return x


@pytest.mark.parametrize("C", [1, 2])
def test_pcm_filters_and_stitch_past_65535_clips(C):
    """pcm16, apply_filters (both compression values, both compressor forms) and stitch of 65 543 clips of a few dozen samples:
    per-clip grids of N x splits blocks and their unsigned casts, against the host functions of audio_util."""
    from riffusion.util import audio_util

    _require(4)
    plan = _plan()
    N, L, rate = GRID_ROWS, 48, 44100
    wave = torch.randn((N * C, L), device="cuda", generator=_gen(21 + C)) * torch.linspace(1e-3, 10.0, N * C, device="cuda")[:, None]
    pcm, peak = plan.pcm16(wave, C)
    for n in GRID_CHECK:
        host = wave[n * C:(n + 1) * C].cpu().numpy()
        assert np.array_equal(pcm[n].cpu().numpy(), audio_util.pcm16_from_waveform(host, normalize=True)), f"pcm16 of clip {n}"
        assert float(peak[n]) == float(np.abs(host).max())

    batch = _pcm_batch(N, L, C, seed=C)
    dev = torch.from_numpy(batch).cuda()
    for compression, form in ((False, "chunked"), (True, "chunked"), (True, "sequential")):
        stats = {}
        got = plan.apply_filters(dev, compression=compression, compress_form=form, stats=stats)
        if compression:
            assert not stats["host_fallback"]
        for n in GRID_CHECK:
            want = audio_util.apply_filters(audio_util.PcmSegment(batch[n], rate), compression=compression)._data
            assert np.array_equal(got[n].cpu().numpy(), want), f"apply_filters(compression={compression}, {form}) of clip {n}"
        del got

    # crossfade 0: stitch_segments is the concatenation (checked on a prefix with the host's own append)
    prefix = audio_util.stitch_segments([audio_util.PcmSegment(c, rate) for c in batch[:5]], 0.0)
    assert np.array_equal(np.asarray(prefix.get_array_of_samples()), batch[:5].reshape(-1))
    got = plan.stitch(dev, rate, 0.0)
    assert got.shape == (N * L, C) and np.array_equal(got.cpu().numpy(), batch.reshape(N * L, C))


# ---- B: slot arrays past 4 GiB and 2^31 elements ----------------------------------------------------------------------------
def _decode_alone(conv, plan, dev_tiles, n, stereo, seed, iters):
    from riffusion.util import image_util

    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    pcm, _ = plan.audio_from_image(dev_tiles[n:n + 1], stereo, lut, iters, 0.99, seed=seed, clip_base=n, magnitude_hint=30e6)
    mel = plan.image_decode(dev_tiles[n:n + 1], stereo, lut)
    C = 2 if stereo else 1
    wave = plan.waveform_from_mel(mel, C, iters, seed=seed, row_base=n * C, magnitude_hint=30e6)
    return pcm, wave.reshape(1, C, -1)


@pytest.mark.parametrize("stereo,tiles,check", [(False, OFFSET_TILES, OFFSET_CHECK), (True, 226, (0, 111, 112, 222, 223, 224, 225))])
def test_decode_past_2_31_slot_elements(stereo, tiles, check):
    """One decode call of 448 mono tiles (226 stereo: 452 rows) at T = 512: the float slots pass 4 GiB of byte offset at row 223
    and 2^31 elements at row 446, the complex ones both at 223.  PCM and float waveforms of the tiles on both sides equal the
    same tile decoded alone at its row_base."""
    from helpers import synthetic_tiles_u8
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter

    _require(36)
    iters, seed = 4, 77
    conv = SpectrogramImageConverter(_params(stereo=stereo, num_griffin_lim_iters=iters), device="cuda")
    plan = conv.converter._plan()
    host_tiles = synthetic_tiles_u8(tiles, seed=tiles + stereo)
    dev_tiles = torch.from_numpy(host_tiles).cuda()
    pcm = conv.audio_from_spectrogram_images(dev_tiles, seed=seed, tiles_per_call=tiles, return_device=True)
    wave = conv.audio_from_spectrogram_images(dev_tiles, seed=seed, tiles_per_call=tiles, return_waveform=True, return_device=True)
    for n in check:
        pcm1, wave1 = _decode_alone(conv, plan, dev_tiles, n, stereo, seed, iters)
        assert torch.equal(pcm[n:n + 1], pcm1), f"PCM of tile {n}"
        assert _same(wave[n:n + 1], wave1), f"waveform of tile {n}"


def test_stft_and_permutations_past_2_31_slot_elements():
    """rfx_stft of 448 clips of 512 frames (float slots 8.6 GB, complex 17 GB): the boundary clips equal the clip alone; then
    unpack_complex / unpack_magnitudes / pack_complex over the whole result against the numpy permutation."""
    _require(40)
    plan = _plan()
    B, Lw = OFFSET_TILES, 441 * 511
    wave = torch.randn((B, Lw), device="cuda", generator=_gen(31)) * 8000.0
    mag, spec, T = plan.stft(wave, True, True)
    assert T == 512
    for c in OFFSET_CHECK + (B - 1,):
        mag1, spec1, _ = plan.stft(wave[c:c + 1], True, True)
        assert _same(mag[c * T:(c + 1) * T], mag1) and _same(spec[c * T:(c + 1) * T], spec1), f"stft of clip {c}"
    del wave
    mags_bft = plan.unpack_magnitudes(mag, B, T)
    for c in OFFSET_CHECK:
        assert _same(mags_bft[c], _unpack_reference(mag[c * T:(c + 1) * T], False)), f"unpack_magnitudes of clip {c}"
    del mag, mags_bft
    kept = {c: spec[c * T:(c + 1) * T].clone() for c in OFFSET_CHECK}
    bft = plan.unpack_complex(spec, B, T)
    del spec
    for c in OFFSET_CHECK:
        assert _same(bft[c], _unpack_reference(kept[c], True)), f"unpack_complex of clip {c}"
    slots = plan.pack_complex(bft)
    for c in OFFSET_CHECK:
        assert _same(slots[c * T:(c + 1) * T], _pack_reference(bft[c], True)), f"pack_complex of clip {c}"


def test_forward_images_of_448_five_second_clips():
    """image_from_waveform of 448 five-second clips in one call: images and maxima of the boundary clips equal the clip alone."""
    from riffusion.util import image_util

    _require(8)
    plan = _plan()
    B, Lw = OFFSET_TILES, 5 * 44100
    wave = torch.randn((B, Lw), device="cuda", generator=_gen(41)) * 8000.0
    thr = plan.device_constant(("encode_thresholds", 0.25), lambda: image_util.encode_thresholds(0.25))
    img, mx = plan.image_from_waveform(wave, False, thr)
    for c in OFFSET_CHECK:
        img1, mx1 = plan.image_from_waveform(wave[c:c + 1], False, thr)
        assert torch.equal(img[c:c + 1], img1) and _same(mx[c:c + 1], mx1), f"clip {c}"
