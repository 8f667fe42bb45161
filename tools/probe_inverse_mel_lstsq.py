"""
Times the closed-form InverseMelScale (rfx_inverse_mel_lstsq) against the SGD (rfx_inverse_mel) on 64 mono tiles of 512 frames,
the product call with inverse_mel="lstsq" against "sgd", and a device-to-device copy of the bytes the expansion writes - all in
one run, medians of 20 event-timed repetitions after 3 warm-up calls.  Then the quality figure: the spectral convergence
(`return_error`) of the five golden tiles and og_beat_64.png with both forms at the same seed, after the default 32 Griffin-Lim
iterations.  Prints plain text (profiles/inverse_mel_lstsq.txt is a copy of it).

    python tools/probe_inverse_mel_lstsq.py [--tiles 64] [--reps 20] [--no-quality]

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probe_inverse_mel_lstsq.py --reps 3 --no-quality`.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "riffusion-hobby_amd"), os.path.join(ROOT, "oracle")]


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()

    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    params = SpectrogramParams()
    conv = SpectrogramImageConverter(params, device="cuda")
    plan = _hip.get_plan(params, "cuda:0")
    B, T = args.tiles, 512
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(rng.integers(0, 256, size=(B, 512, T, 3), dtype=np.uint8)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, False, lut)
    print(f"device {torch.cuda.get_device_name(0)}; {B} mono tiles x {T} frames; medians of {args.reps} (min .. max), ms")

    def row(name, r):
        print(f"  {name:<58s} {r[0]:8.3f}  ({r[1]:.3f} .. {r[2]:.3f})")

    lin = plan.inverse_mel_lstsq(mel)
    row("rfx_inverse_mel_lstsq", timed(lambda: plan.inverse_mel_lstsq(mel), args.reps))
    row("rfx_inverse_mel (SGD, hint 30e6)", timed(lambda: plan.inverse_mel(mel, 1, seed=1, magnitude_hint=30e6), args.reps))
    dst = torch.empty_like(lin)
    r = timed(lambda: dst.copy_(lin), args.reps)
    row(f"device-to-device copy of |S| ({lin.numel() * 4 / 1e9:.2f} GB)", r)
    print(f"    copy rate {2 * lin.numel() * 4 / r[0] / 1e6:.0f} GB/s read + written")
    del dst, lin
    for form in ("lstsq", "sgd"):
        row(f'audio_from_spectrogram_images(inverse_mel="{form}"), device in and out',
            timed(lambda: conv.audio_from_spectrogram_images(tiles, seed=1, return_device=True, inverse_mel=form), args.reps))
    if args.no_quality:
        return
    print("spectral convergence after 32 Griffin-Lim iterations, seed 7 (return_error): tile, sgd, lstsq")
    gold = os.path.join(ROOT, "tests", "golden")
    for name in ("og_beat", "agile", "marim", "motorway", "vibes", "og_beat_64"):
        with Image.open(os.path.join(gold, name + ".png")) as im:
            tile = np.ascontiguousarray(np.asarray(image_util.rgb_array_from_image(im)))[None]
        err = {f: float(conv.audio_from_spectrogram_images(tile, seed=7, return_error=True, inverse_mel=f)[1][0]) for f in ("sgd", "lstsq")}
        print(f"  {name:<12s} {tile.shape[2]:4d} frames   sgd {err['sgd']:.5f}   lstsq {err['lstsq']:.5f}")


if __name__ == "__main__":
    main()
