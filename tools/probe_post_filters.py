"""
What the decode's post-processing costs on the host and on the device (csrc/rfx_pcm.hip).

At the headline size (64 mono tiles of 512 frames) and for one tile:
  decode            audio_from_spectrogram_images(tiles)                       (int16 PCM to the host)
  decode + host     the same, then audio_util.apply_filters clip by clip on the host (what callers did before)
  decode + device   audio_from_spectrogram_images(tiles, apply_filters=True)
and a 36-clip stitch with the audio-to-audio crossfade (0.2 s) of already filtered clips: audio_util.stitch_segments on the host
against Plan.stitch on the device (plus its copy to the host), and the device filters alone (Plan.apply_filters, CUDA events).
Host clock around synchronised calls, after warm-up; medians of `--reps` runs.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import synthetic_tiles_u8  # noqa: E402
from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import audio_util  # noqa: E402


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3)


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def host_filters(pcm, rate):
    return [audio_util.apply_filters(audio_util.PcmSegment(c, rate), compression=False) for c in pcm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    conv = SpectrogramImageConverter(SpectrogramParams(), device="cuda")
    plan = conv.converter._plan()
    rate = conv.p.sample_rate
    res = {"probe": "post_filters", "reps": args.reps}
    for n in (64, 1):
        tiles = synthetic_tiles_u8(n, seed=n)
        res[f"decode_ms_{n}"] = timed(lambda: conv.audio_from_spectrogram_images(tiles, seed=1), args.reps)
        res[f"decode_host_filters_ms_{n}"] = timed(lambda: host_filters(conv.audio_from_spectrogram_images(tiles, seed=1), rate),
                                                   args.reps)
        res[f"decode_device_filters_ms_{n}"] = timed(lambda: conv.audio_from_spectrogram_images(tiles, seed=1, apply_filters=True),
                                                     args.reps)
        pcm = conv.audio_from_spectrogram_images(tiles, seed=1, return_device=True)
        scratch = torch.empty_like(pcm)
        res[f"device_filters_kernels_ms_{n}"] = event_ms(lambda: plan.apply_filters(pcm, out=scratch), args.reps)
    # 36 filtered clips, stitched with the audio-to-audio crossfade
    tiles = synthetic_tiles_u8(36, seed=36)
    pcm = conv.audio_from_spectrogram_images(tiles, seed=2, apply_filters=True, return_device=True)
    host_pcm = pcm.cpu().numpy()
    segs = [audio_util.PcmSegment(c, rate) for c in host_pcm]
    res["stitch36_host_ms"] = timed(lambda: audio_util.stitch_segments(segs, 0.2), max(3, args.reps // 2), warmup=1)
    res["stitch36_device_ms"] = timed(lambda: plan.stitch(pcm, rate, 0.2).cpu(), args.reps)
    res["stitch36_plan_ms"] = timed(lambda: audio_util.stitch_plan(36, pcm.shape[1], rate, 0.2), args.reps)
    same = np.array_equal(plan.stitch(pcm, rate, 0.2).cpu().numpy().reshape(-1), audio_util.stitch_segments(segs, 0.2).get_array_of_samples())
    res["stitch36_same_bytes"] = bool(same)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
