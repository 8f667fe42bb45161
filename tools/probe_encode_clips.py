"""
Encode of one long recording, end to end from the host int16 array to host image bytes: the parent path (host set_frame_rate,
slice_audio_into_clips, spectrogram_image_from_audio per clip) against SpectrogramImageConverter.spectrogram_images_from_audio_clips
(one int16 upload, resample + gather + encode on the device).

    python tools/probe_encode_clips.py [--seconds 240] [--runs 7] [--out profiles/encode_clips_pcm_in.txt]

Workload: a stereo 48 kHz int16 track, 5 s clips overlapping by 0.2 s, mono tiles at 44.1 kHz.  Every figure is the median of
--runs runs after one warm-up; the stages of the device path are timed with events on the stream.  Second part: the resample
kernel's achieved traffic (bytes read + bytes written per second) next to a device-to-device hipMemcpyAsync (torch's copy_ of a
contiguous tensor) that moves the same number of bytes in the same process, for the probe's track and for an hour at 96 kHz.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import audio_util, image_util  # noqa: E402


def make_track(seconds: float, rate: int) -> np.ndarray:
    rng = np.random.default_rng(0)
    t = np.arange(int(seconds * rate)) / rate
    x = np.stack([np.sin(2 * np.pi * 220 * t) * 6000 + np.sin(2 * np.pi * 3301 * t) * 2500, np.sin(2 * np.pi * 330 * t + 1) * 7000], axis=1)
    return (x + rng.normal(0, 900, x.shape)).astype(np.int16)


def median_ms(values):
    return statistics.median(values) * 1e3


def parent_path(conv, seg, starts, duration):
    t0 = time.perf_counter()
    resampled = seg.set_frame_rate(conv.p.sample_rate)
    t1 = time.perf_counter()
    clips = audio_util.slice_audio_into_clips(resampled, starts, duration)
    t2 = time.perf_counter()
    tiles = [np.asarray(conv.spectrogram_image_from_audio(c)) for c in clips]
    t3 = time.perf_counter()
    return tiles, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)


def device_path(conv, seg, starts, duration):
    t0 = time.perf_counter()
    images, _ = conv.spectrogram_images_from_audio_clips(seg, starts, duration)
    tiles = [np.asarray(im) for im in images]
    return tiles, time.perf_counter() - t0


def device_stages(conv, seg, starts, duration):
    """the device path's steps one by one, with an event after each (ms)"""
    plan = conv.converter._plan()
    power = float(conv.p.power_for_image)
    thr = plan.device_constant(("encode_thresholds", power), lambda: image_util.encode_thresholds(power))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    data = np.asarray(seg.get_array_of_samples(), dtype=np.int16).reshape(-1, seg.channels)
    ev[0].record()
    pcm = torch.from_numpy(data).to(plan.device)
    ev[1].record()
    pcm = plan.resample_pcm(pcm, seg.frame_rate, conv.p.sample_rate)
    ev[2].record()
    r = audio_util.clip_frame_ranges(int(pcm.shape[0]), conv.p.sample_rate, starts, duration)
    img, mx = plan.image_from_pcm_clips(pcm, r.starts, r.frames, conv.p.stereo, thr)
    ev[3].record()
    img.cpu(), mx.cpu()
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def timed_gbps(fn, nbytes: int, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rates = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        rates.append(nbytes / (a.elapsed_time(b) * 1e-3) / 1e9)
    return statistics.median(rates)


def resample_bandwidth(plan, frames: int, in_rate: int, out_rate: int, reps: int):
    x = torch.randint(-32768, 32768, (frames, 2), dtype=torch.int16, device=plan.device)
    out = plan.resample_pcm(x, in_rate, out_rate)
    traffic = x.numel() * 2 + out.numel() * 2
    kernel = timed_gbps(lambda: plan.resample_pcm(x, in_rate, out_rate), traffic, reps)
    src = torch.empty(traffic // 2, dtype=torch.uint8, device=plan.device)  # read + written = traffic
    dst = torch.empty_like(src)
    copy = timed_gbps(lambda: dst.copy_(src), traffic, reps)
    return traffic, kernel, copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_clips_pcm_in.txt"))
    args = ap.parse_args()
    assert args.runs >= 5
    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False), device="cuda")
    seg = audio_util.PcmSegment(make_track(args.seconds, 48000), 48000)
    starts = audio_util.clip_start_times(args.seconds, 5.0, 0.2, max_duration_s=args.seconds)
    want, _ = parent_path(conv, seg, starts, 5.0)  # warm-up, and the bytes to hold the device path to
    got, _ = device_path(conv, seg, starts, 5.0)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), "the two paths disagree"
    parent = [parent_path(conv, seg, starts, 5.0)[1] for _ in range(args.runs)]
    device = [device_path(conv, seg, starts, 5.0)[1] for _ in range(args.runs)]
    stages = [device_stages(conv, seg, starts, 5.0) for _ in range(args.runs)]
    p_total, d_total = median_ms([p[3] for p in parent]), median_ms(device)
    lines = [
        f"encode of a {args.seconds:.0f} s stereo 48 kHz int16 track -> {len(starts)} mono tiles (5 s clips, 0.2 s overlap, 44.1 kHz), host int16 -> host image bytes",
        f"device {torch.cuda.get_device_name(0)}, median of {args.runs} runs after warm-up; same image bytes on both paths",
        f"parent path (host set_frame_rate, slice, per-clip spectrogram_image_from_audio): {p_total:9.2f} ms",
        f"    set_frame_rate {median_ms([p[0] for p in parent]):9.2f} ms   slice {median_ms([p[1] for p in parent]):8.2f} ms   "
        f"per-clip encode {median_ms([p[2] for p in parent]):9.2f} ms   (host clock)",
        f"spectrogram_images_from_audio_clips:                                          {d_total:9.2f} ms   ({p_total / d_total:.1f}x)",
        "    device stages (events): upload {:.3f} ms   resample {:.3f} ms   gather + encode {:.3f} ms   download {:.3f} ms".format(
            *[statistics.median(s[i] for s in stages) for i in range(4)]),
    ]
    plan = conv.converter._plan()
    for label, frames, in_rate in ((f"{args.seconds:.0f} s at 48 kHz", int(args.seconds * 48000), 48000), ("3600 s at 96 kHz", 3600 * 96000, 96000)):
        traffic, kernel, copy = resample_bandwidth(plan, frames, in_rate, 44100, 10)
        lines.append(f"resample kernel, stereo {label} -> 44.1 kHz ({traffic / 1e6:.0f} MB read + written): {kernel:7.1f} GB/s; "
                     f"hipMemcpyAsync device-to-device of the same bytes: {copy:7.1f} GB/s ({100 * kernel / copy:.0f} %)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    assert d_total <= p_total, "the device path is slower than the parent path"


if __name__ == "__main__":
    main()
