"""
InverseMelScale wave kernel with the chunks' scalar chains paired (rfx_imel_wave.hip, imel_wave_kernel) on the device:
  * the htk bank (unit form) and the slaney-normalised bank (both weights) take the wave kernel and stay within 1e-5 rel-L2 of the
    group kernels (imel_form="groups", another factorisation of the same SGD);
  * a clip whose targets and start are all zero stops early (its loss is zero at the first step): the scan and the fix-up launch
    re-run it, and every clip of the batch comes out byte for byte as when it is converted alone.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

pytestmark = pytest.mark.gpu

WAVE_KERNEL = 4  # rfx_plan_imel_kernel: one wave per frame


def _mel(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n, 512, 512, generator=g) ** 4 * 3e7).cuda()


@pytest.mark.parametrize("norm", [None, "slaney"])
def test_wave_kernel_tracks_the_group_kernels(norm):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    params = SpectrogramParams(mel_scale_norm=norm)
    wave = _hip.get_plan(params, "cuda")
    groups = _hip.get_plan(params, "cuda", imel_form="groups")
    assert wave.lib.rfx_plan_imel_kernel(wave.handle) == WAVE_KERNEL
    mel = _mel(2, 11)
    a = wave.inverse_mel(mel, 1, seed=4)
    b = groups.inverse_mel(mel, 1, seed=4)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    rel = float(torch.linalg.norm(a - b) / torch.linalg.norm(b))
    print(f"norm={norm!r}: wave vs group kernels rel-L2 {rel:.2e}")
    assert rel < 1e-5


@pytest.mark.parametrize("norm", [None, "slaney"])
def test_early_stop_and_fixup_batch_equals_alone(norm):
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    plan = _hip.get_plan(SpectrogramParams(mel_scale_norm=norm), "cuda")
    mel = _mel(3, 12)
    g = torch.Generator(device="cpu").manual_seed(13)
    spec0 = torch.rand(3, 512, plan.n_stft, generator=g).cuda()
    mel[1].zero_()  # all-zero targets from an all-zero start: the clip's loss is 0 at the first step, the stopping rule fires
    spec0[1].zero_()
    rows = 512
    batch = plan.inverse_mel(mel, 1, spec0=spec0, seed=9)
    for c in range(3):
        alone = plan.inverse_mel(mel[c:c + 1].contiguous(), 1, spec0=spec0[c:c + 1].contiguous(), seed=9, row_base=c)
        torch.cuda.synchronize()
        assert torch.equal(batch[c * rows:(c + 1) * rows].view(torch.int32), alone.view(torch.int32)), f"clip {c}"
    assert not batch[rows:2 * rows].any()  # the stopped clip: nothing moves away from zero
