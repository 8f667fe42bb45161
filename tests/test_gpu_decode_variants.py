"""Every decode variant through the batch entry's three routes, chunked and whole, and through the fused call by hand: one set of
bytes.  What the routes share is one `ClipExtras` lowered per chunk; this is where a slice, a channel row or an option that one route
forgets would show.  Default params, mono and stereo, 5 random tiles of width 48 (the smallest that serves every variant: a loop
needs 40 columns, a plain call 22), 2 Griffin-Lim iterations, a fixed seed; chunks of 2, 2 and 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, W, ITERS, SEED, MAX_VALUE = 5, 48, 2, 11, 30e6
_RNG = np.random.default_rng(20240)
TILES = _RNG.integers(0, 256, size=(N, 512, W, 3), dtype=np.uint8)
GUIDES = (_RNG.standard_normal((N, 1, 21000)) * 3000).astype(np.float32)  # mono: it serves both rows of a stereo tile
MASK = _RNG.random((N, 512, W)) < 0.5
MASK[:, :, :5] = True

VARIANTS = {
    "plain": {},
    "lstsq": dict(inverse_mel="lstsq"),
    "guided": dict(guide_waveforms=GUIDES),
    "guided + hold_frames": dict(guide_waveforms=GUIDES, hold_frames=(3, 2)),
    "guided + band mask": dict(guide_waveforms=GUIDES, hold_mask=MASK),
    "loop": dict(loop=True),
    "loop + guided": dict(loop=True, guide_waveforms=GUIDES),
    "peaks": dict(phase_start="peaks"),
}


@pytest.fixture(scope="module", params=[False, True], ids=["mono", "stereo"])
def conv(request):
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramImageConverter(SpectrogramParams(stereo=request.param), device="cuda")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_routes_chunks_and_the_fused_call_give_one_set_of_bytes(conv, name):
    from riffusion.spectrogram_converter import hold_mask_rows, hold_rows
    from riffusion.util import image_util

    kw = dict(VARIANTS[name], seed=SEED, griffin_lim_iters=ITERS, max_value=MAX_VALUE)
    loop = bool(kw.get("loop"))
    C = 2 if conv.p.stereo else 1
    plan = conv.converter._plan()
    whole = conv.audio_from_spectrogram_images(TILES, tiles_per_call=N, **kw)
    assert whole.dtype == np.int16 and whole.shape == (N, plan.output_samples(W, loop), C) and whole.any()
    want = whole.tobytes()
    # chunks of 2, 2 and 1
    assert conv.audio_from_spectrogram_images(TILES, tiles_per_call=2, **kw).tobytes() == want
    # the waveform route, then `Plan.pcm16`
    wave = conv.audio_from_spectrogram_images(TILES, tiles_per_call=2, return_waveform=True, return_device=True, **kw)
    assert wave.shape == (N, C, whole.shape[1])
    assert plan.pcm16(wave.reshape(N * C, -1), C, normalize=True)[0].cpu().numpy().tobytes() == want
    # the error route
    pcm, errors = conv.audio_from_spectrogram_images(TILES, tiles_per_call=2, **{"return_loop_error" if loop else "return_error": True}, **kw)
    assert pcm.tobytes() == want and errors.shape == (N,) and np.isfinite(errors).all()
    # the fused call on chunk (2, 4), its rows' tensors built here
    a, b, dev = 2, 4, plan.device
    rows = {}
    if "guide_waveforms" in kw:
        g = torch.from_numpy(GUIDES)[a:b].to(dev, torch.float32)
        rows["guide"] = g.expand(b - a, C, g.shape[2]).reshape((b - a) * C, g.shape[2])
    if "hold_frames" in kw:
        rows["hold"] = hold_rows(kw["hold_frames"], N, W)[a:b].to(dev).repeat_interleave(C, 0).contiguous()
    if "hold_mask" in kw:
        bands = hold_mask_rows(MASK, N, plan.n_mels, W)
        rows["hold_bins"] = plan.hold_bins_from_bands(bands[a:b].to(dev)).repeat_interleave(C, 0).contiguous()
    lut = torch.from_numpy(image_util.decode_lut(float(conv.p.power_for_image), MAX_VALUE)).to(dev)
    direct = plan.audio_from_image(torch.from_numpy(TILES[a:b]).to(dev), conv.p.stereo, lut, ITERS, 0.99, seed=SEED, normalize=True, clip_base=a,
                                   magnitude_hint=MAX_VALUE, lstsq=kw.get("inverse_mel") == "lstsq", loop=loop,
                                   peak_start=kw.get("phase_start") == "peaks", **rows)[0]
    assert direct.cpu().numpy().tobytes() == whole[a:b].tobytes()
