"""
Times the backward of the closed-form InverseMelScale (rfx_inverse_mel_lstsq_backward) on 64 mono tiles of 512 frames: the entry
alone; the member's forward + backward (inverse_mel_scaler(..., inverse_mel="lstsq"), which adds the unpack and pack passes) with
their share; the forward entry; a device-to-device copy of the gradient's bytes; and torch's own
relu(torch.linalg.lstsq(fb.T[None], mel, driver="gels").solution) with torch autograd on the same device tensors, time and peak
allocation.  All in one run, medians of 20 event-timed repetitions after 3 warm-up calls.  Prints plain text
(profiles/inverse_mel_lstsq_backward.txt is a copy of it).

    python tools/probe_inverse_mel_lstsq_backward.py [--tiles 64] [--reps 20] [--no-torch]

For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probe_inverse_mel_lstsq_backward.py --reps 3 --no-torch`.
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


def peak_of(fn):
    """peak bytes torch's allocator held above what was live before the call"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()

    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    params = SpectrogramParams()
    conv = SpectrogramConverter(params, device="cuda")
    plan = _hip.get_plan(params, "cuda:0")
    B, T = args.tiles, 512
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(rng.integers(0, 256, size=(B, 512, T, 3), dtype=np.uint8)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, False, lut)
    del tiles
    gx = torch.randn((B, plan.n_stft, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    gx_slots = plan.pack_magnitudes(gx)
    print(f"device {torch.cuda.get_device_name(0)}; {B} mono tiles x {T} frames; medians of {args.reps} (min .. max), ms")

    def row(name, r):
        print(f"  {name:<66s} {r[0]:8.3f}  ({r[1]:.3f} .. {r[2]:.3f})")
        return r[0]

    bwd = row("rfx_inverse_mel_lstsq_backward", timed(lambda: plan.inverse_mel_lstsq_backward(mel, gx_slots), args.reps))
    fwd = row("rfx_inverse_mel_lstsq (the forward entry)", timed(lambda: plan.inverse_mel_lstsq(mel), args.reps))
    print(f"    backward entry / forward entry {bwd / fwd:.2f}")
    dst = torch.empty_like(gx_slots)
    r = timed(lambda: dst.copy_(gx_slots), args.reps)
    row(f"device-to-device copy of the gradient slots ({gx_slots.numel() * 4 / 1e9:.2f} GB)", r)
    print(f"    copy rate {2 * gx_slots.numel() * 4 / r[0] / 1e6:.0f} GB/s read + written")
    del dst
    slots = plan.inverse_mel_lstsq(mel)
    unpack = row("unpack_magnitudes of the forward's slots", timed(lambda: plan.unpack_magnitudes(slots, B, T), args.reps))
    pack = row("pack_magnitudes of the (B, n_stft, T) gradient", timed(lambda: plan.pack_magnitudes(gx), args.reps))
    del slots

    leaf = mel.clone().requires_grad_(True)

    def member():
        leaf.grad = None
        conv.inverse_mel_scaler(leaf, inverse_mel="lstsq").backward(gx)

    both = row('inverse_mel_scaler(inverse_mel="lstsq") forward + backward', timed(member, args.reps))
    print(f"    of which unpack + pack {100 * (unpack + pack) / both:.0f} %, the two entries {100 * (fwd + bwd) / both:.0f} %")
    print(f"    peak allocation above the inputs {peak_of(member) / 1e9:.2f} GB")
    if args.no_torch:
        return
    fbT = plan.melfb.cuda().T[None].contiguous()

    def torch_both():
        leaf.grad = None
        torch.relu(torch.linalg.lstsq(fbT, leaf, driver="gels").solution).backward(gx)

    row("torch relu(lstsq(gels).solution) forward + backward, same tensors", timed(torch_both, max(3, args.reps // 4), warmup=1))
    print(f"    peak allocation above the inputs {peak_of(torch_both) / 1e9:.2f} GB")


if __name__ == "__main__":
    main()
