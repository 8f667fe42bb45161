"""
What apply_filters(compression=True) costs on the device (csrc/rfx_compress.hip), at the headline size (64 mono tiles of 512
frames, Griffin-Lim 32 - BASELINE configs[1]):
  decode + filters          audio_from_spectrogram_images(tiles, apply_filters=True), compression False and True, alternating
                            in the same process (host clock around synchronised calls, medians of `--reps` runs)
  filters alone             Plan.apply_filters on the decoded batch, compression=False, and compression=True in both forms of the
                            recurrence (CUDA events; the compressed path includes its one synchronisation)
  repair rounds / flags     per clip of the decoded batch (chunked form), and the flags with the default margin
  host                      audio_util.apply_filters(PcmSegment, compression=True) per clip (a few clips)
and checks that every device result equals the host's bytes on the clips it times there.  Prints one JSON line.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/probe_compression.py --reps 5`.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-clips", type=int, default=3)
    args = ap.parse_args()
    conv = SpectrogramImageConverter(SpectrogramParams(), device="cuda")
    plan = conv.converter._plan()
    rate = conv.p.sample_rate
    res = {"probe": "compression", "reps": args.reps, "tiles": 64}
    tiles = synthetic_tiles_u8(64, seed=64)

    # decode with filters, compression off / on, alternating
    for _ in range(2):
        conv.audio_from_spectrogram_images(tiles, seed=1, apply_filters=True)
        conv.audio_from_spectrogram_images(tiles, seed=1, apply_filters=True, compression=True)
    t = {False: [], True: []}
    for _ in range(args.reps):
        for comp in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            conv.audio_from_spectrogram_images(tiles, seed=1, apply_filters=True, compression=comp)
            torch.cuda.synchronize()
            t[comp].append((time.perf_counter() - t0) * 1e3)
    res["decode_filters_ms"] = round(statistics.median(t[False]), 3)
    res["decode_filters_compression_ms"] = round(statistics.median(t[True]), 3)

    # the filters alone on the decoded batch
    pcm = conv.audio_from_spectrogram_images(tiles, seed=1, return_device=True)
    scratch = torch.empty_like(pcm)
    res["filters_ms"] = event_ms(lambda: plan.apply_filters(pcm, out=scratch), args.reps)
    for form in ("chunked", "sequential"):
        res[f"filters_compression_{form}_ms"] = event_ms(
            lambda: plan.apply_filters(pcm, out=scratch, compression=True, compress_form=form), args.reps)
    stats = {}
    dev = plan.apply_filters(pcm, compression=True, stats=stats).cpu().numpy()
    rounds = stats["rounds"].cpu().numpy()
    res["repair_rounds"] = {"min": int(rounds.min()), "median": float(np.median(rounds)), "max": int(rounds.max())}
    res["flagged_samples"] = stats["n_flagged"]
    res["host_fallback"] = stats["host_fallback"]

    # the host, and the bytes
    host_pcm = pcm.cpu().numpy()
    ms, same = [], True
    for i in range(args.host_clips):
        t0 = time.perf_counter()
        seg = audio_util.apply_filters(audio_util.PcmSegment(host_pcm[i], rate), compression=True)
        ms.append((time.perf_counter() - t0) * 1e3)
        same = same and np.array_equal(seg._data, dev[i])
    res["host_ms_per_clip"] = round(statistics.median(ms), 1)
    res["same_bytes"] = bool(same)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
