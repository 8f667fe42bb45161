"""
Cost of the spectral-error report: rfx_spectral_error alone, and audio_from_spectrogram_images with and without return_error.

    python tools/probe_quality.py [--tiles 64] [--runs 20] [--out profiles/spectral_error.txt]

Workload: `--tiles` mono 512 x 512 tiles (seeded random bytes, as bench.py's), default parameters (InverseMelScale 200 steps,
Griffin-Lim 32 iterations), tiles and results on the device.  Every figure is the median of --runs runs after warm-up, timed
with events on the stream; the two forms of the product call alternate inside one loop.  The entry is timed whole; its forward
transforms are timed again on their own in the entry's grouping (rfx_stft on the same groups of rows into one buffer), and the
reduction is the difference, next to a device-to-device copy that moves the same number of bytes.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

from riffusion import _hip  # noqa: E402
from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import image_util  # noqa: E402

GROUP_BYTES = 128 << 20  # include/rfx.h: the entry walks the rows in groups of at most this many bytes of magnitudes


def event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, runs: int) -> float:
    fn()
    torch.cuda.synchronize()
    return statistics.median(event_ms(fn) for _ in range(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_error.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    N, T = args.tiles, 512
    conv = SpectrogramImageConverter(SpectrogramParams(), device="cuda")
    plan = conv.converter._plan()
    rng = np.random.default_rng(20240807)
    tiles = torch.from_numpy(rng.integers(0, 256, size=(N, 512, T, 3), dtype=np.uint8)).to(plan.device)

    # ---- the entry alone, on a real decode's two ends
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, False, lut)
    wave, lin_slots = conv.converter._waveform_from_mel(plan, mel, seed=1, channels_per_clip=1, magnitude_hint=30e6, return_slots=True)
    sums = plan.spectral_error(wave, lin_slots, N, T)
    sc = conv.converter.convergence_from_sums(sums[:, 0], sums[:, 1]).cpu().numpy()
    entry = median_ms(lambda: plan.spectral_error(wave, lin_slots, N, T), args.runs)
    group = max(1, min(N, GROUP_BYTES // (T * plan.frame_stride * 4)))
    L = wave.shape[1]
    buf = torch.empty((group * T, plan.frame_stride), dtype=torch.float32, device=plan.device)
    stream = _hip.current_stream(plan.device)

    def transforms():
        for r0 in range(0, N, group):
            rows = min(group, N - r0)
            _hip.check(plan.lib.rfx_stft(plan.handle, wave[r0:r0 + rows].data_ptr(), rows, L, buf.data_ptr(), None, stream))

    fwd = median_ms(transforms, args.runs)
    one_launch = median_ms(lambda: plan.stft(wave, True, False), args.runs)
    read_bytes = 2 * N * T * plan.frame_stride * 4
    src = torch.empty(read_bytes // 2, dtype=torch.uint8, device=plan.device)  # read + written = the reduction's two reads
    dst = torch.empty_like(src)
    copy = median_ms(lambda: dst.copy_(src), args.runs)
    reduce_ms = entry - fwd

    # ---- the product call, the two forms alternating
    def decode(flag: bool):
        return conv.audio_from_spectrogram_images(tiles, seed=7, tiles_per_call=N, return_device=True, return_error=flag)

    plain = decode(False)
    with_err, err = decode(True)
    assert torch.equal(plain, with_err), "return_error changed the PCM"
    torch.cuda.synchronize()
    t_plain, t_err = [], []
    for _ in range(args.runs):
        t_plain.append(event_ms(lambda: decode(False)))
        t_err.append(event_ms(lambda: decode(True)))
    p, e = statistics.median(t_plain), statistics.median(t_err)
    spread = (max(t_plain) - min(t_plain)) / p

    lines = [
        f"spectral error of {N} mono tiles of {T} frames, default parameters; device {torch.cuda.get_device_name(0)}, "
        f"median of {args.runs} runs after warm-up, events on the stream",
        f"rfx_spectral_error ({N} rows, groups of {group} rows, {-(-N // group)} groups):              {entry:8.3f} ms",
        f"    its forward transforms alone (rfx_stft on the same groups):          {fwd:8.3f} ms   (one launch over all rows: {one_launch:.3f} ms)",
        f"    reduction (the difference; reads 2 x {read_bytes / 2e9:.3f} GB):                {reduce_ms:8.3f} ms   {read_bytes / reduce_ms / 1e6:7.1f} GB/s",
        f"    device-to-device copy of the same bytes ({read_bytes / 2e9:.3f} GB read + as many written): {copy:8.3f} ms   {read_bytes / copy / 1e6:7.1f} GB/s   "
        f"(reduction at {100 * copy / reduce_ms:.0f} % of the copy's rate)",
        f"audio_from_spectrogram_images, {N} tiles in one call, device in / device out:   {p:8.3f} ms   (spread of the runs {100 * spread:.1f} %)",
        f"    with return_error=True (separate stages + rfx_spectral_error):       {e:8.3f} ms   (+{e - p:.3f} ms, {100 * (e - p) / p:+.2f} % of the call without it)",
        f"    the entry alone is {100 * entry / p:.2f} % of the call without it",
        f"spectral convergence of the {N} decodes: min {sc.min():.4f}  median {np.median(sc):.4f}  max {sc.max():.4f}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
