"""
Times the guided decode as a layer - waveform_from_mel_amplitudes(mel, guide=clip, inverse_mel="lstsq", griffin_lim_iters=0), forward
+ backward - on 64 mono tiles of 512 frames against the chain it replaces, in the same run:
inverse_mel_scaler(inverse_mel="lstsq") -> torch.polar(x, spectrogram_func(clip).angle()) -> waveform_from_spectrogram, forward +
backward, with the clip's phase formed in every step (paired data: each batch brings its own clips) and with it formed once
outside.  Time and peak allocation for each; the two backward entries and the forward call alone; and a device-to-device copy of
the bytes the projection kernel moves (two complex cubes read, one real cube written).  Medians of event-timed repetitions after
warm-up calls, the two forms alternating.  Prints plain text (profiles/guided_decode_backward.txt is a copy of it).

    python tools/probe_guided_backward.py [--tiles 64] [--reps 10] [--no-chain]

For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/probe_guided_backward.py --reps 3 --no-chain`.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "riffusion-hobby_amd"), os.path.join(ROOT, "oracle")]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fns, reps, warmup=2):
    """(median, min, max) per callable; the callables alternate inside every repetition"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(event_ms(fn))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-chain", action="store_true")
    args = ap.parse_args()

    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import image_util

    params = SpectrogramParams()
    conv = SpectrogramConverter(params, device="cuda")
    plan = _hip.get_plan(params, "cuda:0")
    B, T = args.tiles, 512
    L = plan.output_samples(T)
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(rng.integers(0, 256, size=(B, 512, T, 3), dtype=np.uint8)).cuda()
    lut = plan.device_constant(("decode_lut", 0.25, 30e6), lambda: image_util.decode_lut(0.25, 30e6))
    mel = plan.image_decode(tiles, False, lut)
    del tiles
    gen = torch.Generator(device="cuda").manual_seed(1)
    clip = 0.1 * torch.randn((B, L), device="cuda", generator=gen)
    g_w = torch.randn((B, L), device="cuda", generator=gen)
    print(f"device {torch.cuda.get_device_name(0)}; {B} mono tiles x {T} frames, {L} samples per row; medians of {args.reps} (min .. max), ms")

    def row(name, r):
        print(f"  {name:<78s} {r[0]:8.3f}  ({r[1]:.3f} .. {r[2]:.3f})")
        return r[0]

    leaf = mel.clone().requires_grad_(True)

    def member():
        leaf.grad = None
        conv.waveform_from_mel_amplitudes(leaf, guide=clip, inverse_mel="lstsq", griffin_lim_iters=0).backward(g_w)

    def chain(phase=None):
        leaf.grad = None
        if phase is None:
            phase = conv.spectrogram_func(clip).angle()
        x = conv.inverse_mel_scaler(leaf, inverse_mel="lstsq")
        conv.waveform_from_spectrogram(torch.polar(x, phase)).backward(g_w)

    if args.no_chain:
        (m,) = timed([member], args.reps)
        row("the member, forward + backward", m)
    else:
        fixed = conv.spectrogram_func(clip).angle()
        m, c, cf = timed([member, chain, lambda: chain(fixed)], args.reps)
        row("the member, forward + backward", m)
        row("the composed chain, forward + backward, the clip's phase formed in the step", c)
        row("the composed chain, forward + backward, the clip's phase formed once outside", cf)
        print(f"    member / chain {m[0] / c[0]:.2f} (phase in the step), {m[0] / cf[0]:.2f} (phase outside)")
        del fixed
        print(f"  peak allocation above the inputs: the member {peak_of(member) / 1e9:.2f} GB, the chain {peak_of(chain) / 1e9:.2f} GB "
              f"(phase in the step; the phase tensor alone is {B * plan.n_stft * T * 4 / 1e9:.2f} GB)")
    mel_d = mel
    fwd, fused, stage, lsq = timed([lambda: plan.waveform_from_mel(mel_d, B, 0, 0.99, lstsq=True, guide=clip),
                                    lambda: plan.waveform_from_mel_guided_backward(mel_d, clip, g_w),
                                    lambda: plan.griffinlim_guided_backward(clip, g_w, T),
                                    lambda: plan.istft_backward(g_w, B, T)], args.reps)
    row("rfx_waveform_from_mel_ex (lstsq, guided, 0 iterations): the forward call", fwd)
    row("rfx_waveform_from_mel_guided_backward: the fused backward entry", fused)
    row("rfx_griffinlim_guided_backward: the stage entry", stage)
    row("rfx_istft_backward alone (G of the same g_w)", lsq)
    frames, stride = B * T, plan.frame_stride
    moved = frames * stride * (8 + 8 + 4)
    src = torch.empty(moved // 8, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    (cp,) = timed([lambda: dst.copy_(src)], args.reps)
    row(f"device-to-device copy moving the projection's bytes ({moved / 1e9:.2f} GB read + written)", cp)
    print(f"    copy rate {moved / cp[0] / 1e6:.0f} GB/s read + written; the projection kernel's own time: the per-kernel split")


if __name__ == "__main__":
    main()
