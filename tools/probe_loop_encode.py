"""
The loop encode against the plain encode: what the circular forward transform costs, and what a loop decode's circular spectral
convergence is, on the device.

    python tools/probe_loop_encode.py [--runs 15] [--calls 20] [--out profiles/loop_encode.txt]     (on the GPU)

* Time: 64 mono clips of 512 hops (225 792 samples at the default parameters: a 5.12 s loop) through `Plan.image_from_waveform(loop=True)`
  (rfx_image_from_waveform_loop: 512 columns), and in the same run the same clips one sample longer through the unchanged plain entry
  (rfx_image_from_waveform: 513 columns), and - to tell the transform from the shape - the plain entry on the clips cut to 511 hops
  (512 columns, the loop call's frame count).  A sample is --calls calls back to back between two events; median of --runs samples
  after a warm-up of all three, the three alternating.  The loop call does the plain call's arithmetic on 512 / 513 of its frames;
  the ratios are stated per call and per column.
* Error: the loop decode of the five golden seed tiles (tests/golden/agile.png, marim.png, motorway.png, og_beat.png, vibes.png, full
  width) at 32 iterations, seed 7, with `return_loop_error=True`: each clip's circular spectral convergence (rfx_spectral_error_loop).
No bound is fixed in advance; the figures are stated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

TILES = ("agile", "marim", "motorway", "og_beat", "vibes")
SEED, BATCH, COLUMNS, ITERS = 7, 64, 512, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_encode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image

    from riffusion import _hip
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    assert torch.cuda.is_available(), "this probe measures on the GPU"

    def event_ms(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.calls

    p = SpectrogramParams(num_griffin_lim_iters=ITERS)
    plan = _hip.get_plan(p, "cuda")
    P = COLUMNS * p.hop_length
    rng = np.random.default_rng(SEED)
    longer = torch.from_numpy((rng.standard_normal((BATCH, P + 1)) * 8000).astype(np.float32)).cuda()
    clips = longer[:, :P].contiguous()
    shorter = longer[:, :P - p.hop_length].contiguous()
    thr = plan.device_constant(("encode_thresholds", 0.25), lambda: image_util.encode_thresholds(0.25))
    calls = {"loop": lambda: plan.image_from_waveform(clips, False, thr, loop=True), "plain": lambda: plan.image_from_waveform(longer, False, thr),
             "plain512": lambda: plan.image_from_waveform(shorter, False, thr)}
    shapes = {key: tuple(f()[0].shape) for key, f in calls.items()}
    assert shapes["loop"][2] == COLUMNS == shapes["plain512"][2] and shapes["plain"][2] == COLUMNS + 1
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    samples = {key: [] for key in calls}
    for _ in range(args.runs):
        for key, f in calls.items():
            samples[key].append(event_ms(f))
    ms = {key: statistics.median(v) for key, v in samples.items()}
    spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in samples.items()}
    ratio = ms["loop"] / ms["plain"]
    per_column = (ms["loop"] / COLUMNS) / (ms["plain"] / (COLUMNS + 1))
    same_shape = ms["loop"] / ms["plain512"]

    conv = SpectrogramImageConverter(p, device="cuda")
    tiles = np.stack([np.array(Image.open(os.path.join(ROOT, "tests", "golden", name + ".png")).convert("RGB")) for name in TILES])
    assert tiles.shape[2] == COLUMNS
    pcm, err = conv.audio_from_spectrogram_images(tiles, seed=SEED, loop=True, return_loop_error=True)
    assert pcm.shape[1] == P

    lines = [
        f"---- loop encode against the plain encode: {BATCH} mono clips of {COLUMNS} hops ({P} samples), default parameters; device {torch.cuda.get_device_name(0)}",
        f"time: Plan.image_from_waveform, {args.calls} calls back to back per sample, median of {args.runs} samples after warm-up, events on the stream, the "
        "three alternating (spread = (max - min) / median)",
        "",
        f"loop   (rfx_image_from_waveform_loop, {P} samples -> {shapes['loop'][2]} columns): {ms['loop']:8.3f} ms ({100 * spread['loop']:4.1f} %)",
        f"plain  (rfx_image_from_waveform,      {P + 1} samples -> {shapes['plain'][2]} columns): {ms['plain']:8.3f} ms ({100 * spread['plain']:4.1f} %)",
        f"plain  (rfx_image_from_waveform,      {P - p.hop_length} samples -> {shapes['plain512'][2]} columns): {ms['plain512']:8.3f} ms ({100 * spread['plain512']:4.1f} %)",
        f"loop / plain of one sample more: {ratio:.4f} per call, {per_column:.4f} per column; loop / plain of the same {COLUMNS} columns: {same_shape:.4f}",
        "",
        f"circular spectral convergence of the loop decode (audio_from_spectrogram_images(loop=True, return_loop_error=True), {ITERS} iterations, seed {SEED}):",
    ]
    for name, e in zip(TILES, np.asarray(err, np.float64)):
        lines.append(f"{name:10s} {e:.6f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
