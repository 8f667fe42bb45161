"""
What the closed-form InverseMelScale's tests share (TEST INFRASTRUCTURE ONLY; tests/test_imel_lstsq_cpu.py, tests/test_gpu_imel_lstsq.py
and the tests of its gradient and of the guided decode's): a bank and the library's report of it, the host emulator
(csrc/rfx_imel_lstsq_core.h compiled for the host with tests/emu/rfx_imel_lstsq_emu.cpp), built once per process, torch's lstsq as
the reference, and the distance from it.
"""
import ctypes
import functools

import numpy as np
import torch

import emu_build

EMU_SRC = "rfx_imel_lstsq_emu.cpp"


@functools.lru_cache(maxsize=1)
def emulator():
    lib = ctypes.CDLL(emu_build.shared(EMU_SRC, "-ffp-contract=off"))
    lib.emu_inverse_mel_lstsq.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    return lib


def bank(**kw):
    """(oracle params, rfx_params, filterbank (n_stft, n_mels) float32) of a SpectrogramParams variation"""
    import riffusion_oracle as O
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    op = O.params_from(SpectrogramParams(**kw))
    cp = _hip.RfxParams(op.sample_rate, op.n_fft, op.win_length, op.hop_length, op.num_frequencies, op.max_mel_iters)
    return op, cp, O.mel_filterbank(op).to(torch.float32).contiguous()


def report(cp, fb, tables=False):
    from riffusion import _hip

    return _hip.lstsq_bank_report(cp, fb, tables=tables)


def emu_run(emu, fb, tables, mel):
    """mel (B, M, T) float32 tensor -> (B, F, T) float32 tensor by the emulator"""
    neg_l, inv_d = tables
    F, M = fb.shape
    B, M2, T = mel.shape
    assert M2 == M, (M2, M)
    mel = np.ascontiguousarray(mel.numpy(), dtype=np.float32)
    fbn = np.ascontiguousarray(fb.numpy(), dtype=np.float32)
    out = np.full((B, F, T), np.nan, np.float32)
    emu.emu_inverse_mel_lstsq(fbn.ctypes.data, neg_l.ctypes.data, inv_d.ctypes.data, mel.ctypes.data, B, F, M, T, None, out.ctypes.data)
    return torch.from_numpy(out)


def lstsq_reference(fb, mel, dtype):
    return torch.relu(torch.linalg.lstsq(fb.T[None].to(dtype), mel.to(dtype), driver="gels").solution)


def distances(x, ref):
    """relative L2 distance of x from ref (B, F, T): overall, and of the worst single frame"""
    diff, ref = x.double() - ref, ref
    per_frame = diff.norm(dim=1) / ref.norm(dim=1)
    return float(diff.norm() / ref.norm()), float(per_frame.max())


def image_mel(M, T, max_value=30e6, seed=3):
    """a uniform-random uint8 tile decoded as the image path does: not in the range of fb^T"""
    import riffusion_oracle as O

    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(M, T, 3), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(O.spectrogram_from_image_u8(img, max_value=max_value, stereo=False))).to(torch.float32)


# the device tests' banks: name -> (SpectrogramParams keywords, B, T)
DEVICE_CASES = {
    "default": (dict(), 3, 37),
    "norm_slaney": (dict(mel_scale_norm="slaney"), 3, 37),
    "8khz_64": (dict(sample_rate=8000, num_frequencies=64, max_frequency=4000), 2, 21),
}
CANARY = 4096


def _params(**kw):
    from riffusion.spectrogram_params import SpectrogramParams

    return SpectrogramParams(**kw)


def _plan(**kw):
    from riffusion import _hip

    return _hip.get_plan(_params(**kw), "cuda:0")


def _bits(t: torch.Tensor) -> bytes:
    return t.detach().cpu().contiguous().numpy().tobytes()


def _mel(M, B, T, max_value=30e6, seed=3):
    """B random uint8 tiles decoded as the image path does (B, M, T)"""
    return torch.cat([image_mel(M, T, max_value=max_value, seed=seed + i) for i in range(B)]).contiguous()
