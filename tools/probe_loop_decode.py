"""
Loop decode against the plain decode of the same tiles: the step at the loop point, and the time of the Griffin-Lim call.

    python tools/probe_loop_decode.py [--runs 9] [--out profiles/loop_decode.txt]     (on the GPU)

Workload: the five golden seed tiles (tests/golden/agile.png, marim.png, motorway.png, og_beat.png, vibes.png) at their full width of
512 columns, default parameters, 32 Griffin-Lim iterations, seed 7.

* Seam figure (tests/loop_oracle.py): |x[0] - x[-1]| over the RMS sample-to-sample step of the clip, of the float waveform
  `audio_from_spectrogram_images(return_waveform=True)` gives - with loop=True and without - per tile.
* Time of `Plan.griffinlim` on the tiles' linear magnitudes (InverseMelScale run once, outside the timing) for 1 tile and for 64 (the
  five tiles in turn), median of --runs runs after a warm-up, events on the stream, the forms alternating:
      loop     loop=True (always the per-frame form);
      frames   the unlooped call on a plan forced to the per-frame form (gl_form="frames"): the same frame kernel and one fold each.
  The unlooped kernels of this commit are the parent commit's, instruction for instruction (the ISA of every existing kernel compares
  equal), so `frames` is measured here, in the same process and on the same box as `loop`.
No bound is fixed for the ratio; it is stated, and explained where it leaves the box-to-box spread of 3 %.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILES = ("agile", "marim", "motorway", "og_beat", "vibes")
N_ITER, SEED = 32, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image

    import loop_oracle
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

    looped = conv.audio_from_spectrogram_images(tiles, seed=SEED, return_waveform=True, loop=True)
    plain = conv.audio_from_spectrogram_images(tiles, seed=SEED, return_waveform=True)
    assert looped.shape == (n, 1, p.hop_length * T) and plain.shape == (n, 1, p.hop_length * (T - 1))
    seam_loop, seam_plain = loop_oracle.seam_figure(looped[:, 0]), loop_oracle.seam_figure(plain[:, 0])

    auto, frames = _hip.get_plan(p, "cuda"), _hip.get_plan(p, "cuda", gl_form="frames")
    lut = auto.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    times = {}
    for B in (1, 64):
        batch = torch.from_numpy(tiles[[i % n for i in range(B)]]).cuda()
        S = auto.inverse_mel(auto.image_decode(batch, False, lut), 1, seed=SEED)
        forms = {"loop": lambda: auto.griffinlim(S, B, T, N_ITER, 0.99, seed=SEED, loop=True),
                 "frames": lambda: frames.griffinlim(S, B, T, N_ITER, 0.99, seed=SEED)}
        for f in forms.values():
            f()
        torch.cuda.synchronize()
        samples = {k: [] for k in forms}
        for _ in range(args.runs):
            for k, f in forms.items():
                samples[k].append(event_ms(f))
        for k in forms:
            times[(B, k)] = (statistics.median(samples[k]), (max(samples[k]) - min(samples[k])) / statistics.median(samples[k]))

    lines = [
        f"---- loop decode of the five golden seed tiles ({', '.join(TILES)}; mono, {T} columns), default parameters, {N_ITER} Griffin-Lim iterations, seed {SEED}; "
        f"device {torch.cuda.get_device_name(0)}",
        "seam figure = |x[0] - x[-1]| over the RMS sample-to-sample step of the clip, of the float waveform (1 = an ordinary step)",
        "",
        "tile        loop decode   plain decode of the same tile",
    ]
    for i, name in enumerate(TILES):
        lines.append(f"{name:10s}  {seam_loop[i]:11.2f}   {seam_plain[i]:11.2f}")
    lines += [
        f"{'mean':10s}  {float(seam_loop.mean()):11.2f}   {float(seam_plain.mean()):11.2f}",
        "",
        f"Plan.griffinlim on the tiles' linear magnitudes, {N_ITER} iterations; median of {args.runs} runs after warm-up, events on the stream, the two forms alternating",
        "`loop` is the loop call (per-frame form), `frames` the unlooped call on a plan forced to the per-frame form (gl_form = frames); the unlooped kernels are the "
        "parent commit's instruction for instruction",
        "",
        "tiles   loop ms (spread)    frames ms (spread)   loop / frames",
    ]
    for B in (1, 64):
        (tl, sl), (tf, sf) = times[(B, "loop")], times[(B, "frames")]
        lines.append(f"{B:5d}   {tl:8.3f} ({100 * sl:4.1f} %)   {tf:8.3f} ({100 * sf:4.1f} %)    {tl / tf:.3f}")
    lines += [
        "",
        "A loop call folds T hop blocks per row where the unlooped call folds T - 1, and its fold sums one chain of ten frames per sample without the clamp at the "
        "clip's ends or the group split; the frame kernel differs in the index rule of its ten input loads alone.",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
