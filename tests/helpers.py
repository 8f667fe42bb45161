"""Shared helpers of the test-suite (seeded synthetic inputs of SURVEY.md 8(d), SNR)."""
import os

import numpy as np
import torch


def oracle():
    """the CPU oracle (oracle/riffusion_oracle.py), with torch's thread pool sized for the comparisons the tests run on it"""
    import riffusion_oracle

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return riffusion_oracle


def snr_db(ref: torch.Tensor, x: torch.Tensor) -> float:
    ref = ref.double().flatten()
    x = x.double().flatten()
    return float(10.0 * torch.log10(ref.pow(2).sum() / (ref - x).pow(2).sum().clamp_min(1e-300)))


def synthetic_tiles_u8(batch: int, height: int = 512, width: int = 512, seed: int = 20240807) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(batch, height, width, 3), dtype=np.uint8)


def synthetic_wave(batch: int, length: int, seed: int = 20240807) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal((batch, length)) * 8000).astype(np.float32))


def smooth_magnitudes(batch: int, n_stft: int, frames: int, seed: int = 7) -> torch.Tensor:
    """Magnitude spectrogram of a synthetic signal: gives Griffin-Lim something consistent to chew."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, n_stft, frames, generator=g) * 1000.0


def mask_ill_conditioned_bins(O, mag: torch.Tensor, op, angles0: torch.Tensor, n_iter: int, rel: float = 1e-4, passes: int = 4):
    """
    Griffin-Lim's phase update normalises `a = rebuilt - m * tprev` bin by bin; where |a| is nearly zero the new phase is
    decided by rounding, on every implementation (profiles/r04_griffinlim_one_bin_events.txt: a 60 dB result after four
    iterations is ONE bin of one frame).  This finds those bins with the oracle in float64 - |a| < rel x the frame's largest
    |a| in any of the first n_iter iterations - and returns the magnitudes with them set to ZERO: a bin of magnitude zero
    contributes Z = 0 whatever its phase, so device and oracle can be compared on the same, now well-conditioned problem
    (zeroing changes the trajectory, so the scan is repeated until it comes back clean).
    Returns (masked magnitudes, number of masked (clip, bin, frame) entries).
    """
    mag = mag.clone()
    total = 0
    for _ in range(passes):
        bad = torch.zeros(mag.shape, dtype=torch.bool)

        def watch(k, a):
            small = a.abs() < rel * a.abs().amax(dim=-2, keepdim=True)
            bad.logical_or_(small & (mag > 0))

        O.griffinlim(mag, op, angles0=angles0, n_iter=n_iter, dtype=torch.float64, on_update=watch)
        n = int(bad.sum())
        if n == 0:
            break
        mag[bad] = 0.0
        total += n
    return mag, total


# option fields of `need` for a guided call, one with held frames and a masked one: dummy aligned addresses, a guide row of one sample
GUIDE = dict(d_guide=0x1000, guide_stride=1, guide_samples=1)
HELD = dict(GUIDE, d_hold_frames=0x1000)
MASKED = dict(GUIDE, d_hold_bins=0x1000)


def need(lib, entry: str, plan_handle, *shape: int, **fields) -> int:
    """The workspace of a call of `entry` ("griffinlim", "waveform_from_mel", "audio_from_image") with the options `fields`
    (rfx_start_call_options' own names; pointers as addresses, which the library never dereferences here): the entry's
    rfx_*_workspace_bytes_ex query.  0 with the refusal in rfx_last_error for options the entry refuses."""
    import ctypes

    from riffusion import _hip

    opt = _hip.RfxStartCallOptions(struct_size=ctypes.sizeof(_hip.RfxStartCallOptions), **fields)
    return getattr(lib, f"rfx_{entry}_workspace_bytes_ex")(plan_handle, *shape, ctypes.byref(opt))


def queries_refuse(lib, opt, word: bytes) -> bool:
    """Each of the three rfx_*_workspace_bytes_ex queries answers 0 for the ctypes options `opt` (no plan is needed: the options are
    read first) and leaves a refusal with `word` in rfx_last_error under its own name."""
    import ctypes

    for name, shape in (("rfx_griffinlim_workspace_bytes_ex", (1, 30)), ("rfx_waveform_from_mel_workspace_bytes_ex", (1, 30)),
                        ("rfx_audio_from_image_workspace_bytes_ex", (1, 0, 30))):
        if getattr(lib, name)(None, *shape, ctypes.byref(opt)) != 0 or not lib.rfx_last_error().startswith(name.encode() + b": "):
            return False
        if word not in lib.rfx_last_error():
            return False
    return True


def plan_bank_report(op, fb="oracle", frame_engine: str = "auto", plan_layout: str = "auto", imel_form: str = "auto"):
    """rfx_debug_plan_bank (include/rfx.h, no GPU): what rfx_plan_create_ex decides for the oracle parameter set `op`, its
    filterbank as the oracle builds it (or the (n_stft, n_mels) float32 tensor `fb`, or None for a plan without one) and the
    given plan options.  Raises RfxError where plan creation refuses the geometry."""
    import ctypes

    import riffusion_oracle as O
    from riffusion import _hip

    lib = _hip.load_library()
    if isinstance(fb, str):
        fb = O.mel_filterbank(op)
    if fb is not None:
        fb = fb.to(torch.float32).contiguous()
        assert tuple(fb.shape) == (op.n_stft, op.num_frequencies)
    cp = _hip.RfxParams(op.sample_rate, op.n_fft, op.win_length, op.hop_length, op.num_frequencies, op.max_mel_iters)
    opt = _hip.RfxPlanOptions(ctypes.sizeof(_hip.RfxPlanOptions), 0, 0, _hip.FRAME_ENGINES[frame_engine], _hip.PLAN_LAYOUTS[plan_layout],
                              _hip.IMEL_FORMS[imel_form])
    report = _hip.RfxPlanBankReport(struct_size=ctypes.sizeof(_hip.RfxPlanBankReport))
    _hip.check(lib.rfx_debug_plan_bank(ctypes.byref(cp), fb.data_ptr() if fb is not None else None, ctypes.byref(opt), ctypes.byref(report)))
    return report
