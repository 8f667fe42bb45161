"""
The spectral-peak start of Griffin-Lim against the random start: what it costs and what it saves, on the device.

    python tools/probe_peak_start.py [--runs 9] [--out profiles/peak_start.txt]     (on the GPU)

Workload: 64 tiles - the five golden seed tiles (tests/golden/agile.png, marim.png, motorway.png, og_beat.png, vibes.png) in turn, at
their full width of 512 columns - default parameters, seed 7.

* Time of `Plan.griffinlim` on the tiles' linear magnitudes (InverseMelScale run once, outside the timing) at 0 / 2 / 4 / 8 / 16 / 32
  iterations with peak_start=True and with the random start: median of --runs runs after a warm-up of every shape, events on the
  stream, the two starts alternating.  The start's own time: `Plan.peak_start` on the same magnitudes, timed the same way, and stated
  in Griffin-Lim iterations of the same batch ((random at 32 - random at 0) / 32).
* Mean spectral convergence over the five tiles of `audio_from_spectrogram_images(return_error=True)` at the same iteration counts,
  for both starts.
* The comparison that decides whether the start pays: peaks at k iterations against random at 2 k - time and error side by side.
No bound is fixed in advance; the figures are stated.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

TILES = ("agile", "marim", "motorway", "og_beat", "vibes")
ITERS = (0, 2, 4, 8, 16, 32)
SEED, BATCH = 7, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peak_start.txt"))
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
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    p = SpectrogramParams()
    conv = SpectrogramImageConverter(p, device="cuda")
    tiles = np.stack([np.array(Image.open(os.path.join(ROOT, "tests", "golden", name + ".png")).convert("RGB")) for name in TILES])
    n, _, T, _ = tiles.shape
    assert T == 512

    # quality: the product path, the five tiles
    sc = {}
    for k in ITERS:
        for start in ("peaks", "random"):
            _, err = conv.audio_from_spectrogram_images(tiles, seed=SEED, griffin_lim_iters=k, phase_start=start, return_error=True)
            sc[(start, k)] = np.asarray(err, np.float64)

    # time: Plan.griffinlim on 64 tiles' magnitudes
    plan = _hip.get_plan(p, "cuda")
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    batch = torch.from_numpy(tiles[[i % n for i in range(BATCH)]]).cuda()
    S = plan.inverse_mel(plan.image_decode(batch, False, lut), 1, seed=SEED)
    calls = {("start", -1): lambda: plan.peak_start(S, BATCH, T)}
    for k in ITERS:
        calls[("peaks", k)] = lambda k=k: plan.griffinlim(S, BATCH, T, k, 0.99, seed=SEED, peak_start=True)
        calls[("random", k)] = lambda k=k: plan.griffinlim(S, BATCH, T, k, 0.99, seed=SEED)
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    samples = {key: [] for key in calls}
    for _ in range(args.runs):
        for key, f in calls.items():
            samples[key].append(event_ms(f))
    ms = {key: statistics.median(v) for key, v in samples.items()}
    spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in samples.items()}
    per_iter = (ms[("random", 32)] - ms[("random", 0)]) / 32
    start_ms = ms[("start", -1)]

    lines = [
        f"---- spectral-peak start against the random start: {BATCH} tiles (the five golden seed tiles {', '.join(TILES)} in turn; mono, {T} columns), default "
        f"parameters, seed {SEED}; device {torch.cuda.get_device_name(0)}",
        f"time: Plan.griffinlim on the tiles' linear magnitudes, median of {args.runs} runs after warm-up, events on the stream, the starts alternating (spread = "
        "(max - min) / median)",
        "error: mean spectral convergence of the five tiles, audio_from_spectrogram_images(return_error=True)",
        "",
        "n_iter   peaks ms (spread)   random ms (spread)   peaks - random ms   error peaks   error random",
    ]
    for k in ITERS:
        tp, tr = ms[("peaks", k)], ms[("random", k)]
        lines.append(f"{k:6d}   {tp:8.3f} ({100 * spread[('peaks', k)]:4.1f} %)   {tr:8.3f} ({100 * spread[('random', k)]:4.1f} %)   {tp - tr:17.3f}   "
                     f"{float(sc[('peaks', k)].mean()):11.4f}   {float(sc[('random', k)].mean()):12.4f}")
    lines += [
        "",
        "per tile, error peaks / random:",
    ]
    for i, name in enumerate(TILES):
        lines.append(f"{name:10s} " + "   ".join(f"{k}: {sc[('peaks', k)][i]:.4f} / {sc[('random', k)][i]:.4f}" for k in ITERS))
    lines += [
        "",
        f"the start alone (Plan.peak_start, three launches): {start_ms:.3f} ms ({100 * spread[('start', -1)]:.1f} %); one Griffin-Lim iteration of the same batch "
        f"((random at 32 - random at 0) / 32): {per_iter:.3f} ms; the start costs {start_ms / per_iter:.2f} iterations",
        "",
        "peaks at k against random at 2 k (does the start pay for itself?):",
        "     k   peaks at k: ms, error    random at 2k: ms, error",
    ]
    for k in (2, 4, 8, 16):
        lines.append(f"{k:6d}   {ms[('peaks', k)]:8.3f}  {float(sc[('peaks', k)].mean()):.4f}        {ms[('random', 2 * k)]:8.3f}  {float(sc[('random', 2 * k)].mean()):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
