"""
Time stretch: the kernel against a copy of the same bytes, the fused entry, the member, and the torch composition it replaces.

    python tools/probe_time_stretch.py [--rows 64] [--frames 512] [--runs 9] [--out profiles/time_stretch.txt]     (on the GPU)

Workload: `--rows` rows of `--frames` frames at the default parameters (seeded noise of hop * (frames - 1) samples), at rate 1.25 and
at rate 0.8.  Every figure is the median of --runs runs after a warm-up of the same shape, device events on the stream around one
call, the routes of a rate alternating.  Recorded, not gated:
    kernel        rfx_phase_vocoder on a spectrogram in slot layout into a preallocated result.  Bytes: the frames it reads plus the
                  frames it writes, (T + T_out) * rows * frame_stride * 8, over its time; beside it a device-to-device copy that
                  moves the same bytes (half of them read, half written) and the ratio of the two times.
    plan          Plan.time_stretch: rfx_stft -> kernel -> rfx_istft on row groups, waveform to waveform.
    member        SpectrogramConverter.time_stretch on the same device tensor.
    torch         the composition a user writes today on (B, n_stft, T) tensors: spectrogram_func -> the float32 transcription of
                  torchaudio's phase_vocoder (tests/vocoder_oracle.py) on the device -> waveform_from_spectrogram.
    peak          torch.cuda.max_memory_allocated over one call of the member and of the torch route, above what was allocated before.
    one row       the kernel on ONE row of `--frames` frames: the latency case - frame_stride threads walk T_out steps - beside the
                  batch's time per row; where it is more than four times that, the file says so and names the next step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("riffusion-hobby_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

RATES = (1.25, 0.8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_stretch.txt"))
    args = ap.parse_args()

    import torch

    import vocoder_oracle as VO
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    assert torch.cuda.is_available(), "this probe measures on the GPU"
    p = SpectrogramParams()
    conv = SpectrogramConverter(p, device="cuda")
    plan = conv._plan()
    B, T, fs = args.rows, args.frames, plan.frame_stride
    Lw = p.hop_length * (T - 1)
    wave = (torch.randn(B, Lw, generator=torch.Generator().manual_seed(5)) * 8000).cuda()
    _, spec, Tn = plan.stft(wave, want_mag=False, want_spec=True)
    assert Tn == T
    stream = torch.cuda.current_stream().cuda_stream

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def medians(routes):
        """{name: median ms}: a warm-up of every route, then --runs rounds, the routes alternating inside a round"""
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():
                times[name].append(event_ms(fn))
        return {name: statistics.median(v) for name, v in times.items()}, {name: (min(v), max(v)) for name, v in times.items()}

    def peak_above(fn):
        torch.cuda.synchronize()
        plan.release_workspaces()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak

    def torch_route(w, rate):
        X = conv.spectrogram_func(w)
        return conv.waveform_from_spectrogram(VO.phase_vocoder(X, rate, p.hop_length, torch.float32))

    lines = [f"time stretch on {torch.cuda.get_device_name(0)}: {B} rows of {T} frames ({Lw} samples), default parameters, frame_stride {fs}; "
             f"medians of {args.runs} runs (min .. max), device events around one call"]
    for rate in RATES:
        Tout = _hip.phase_vocoder_frames(T, rate)
        out = torch.empty((B * Tout, fs), dtype=torch.complex64, device="cuda")
        nbytes = (T + Tout) * B * fs * 8
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        spec1, out1 = spec[:T], out[:Tout]

        def kernel(rows=B, x=spec, y=out):
            _hip.check(plan.lib.rfx_phase_vocoder(plan.handle, x.data_ptr(), rows, T, rate, y.data_ptr(), stream))

        med, spread = medians({
            "kernel": kernel,
            "copy": lambda: dst.copy_(src),
            "one row": lambda: kernel(1, spec1, out1),
            "plan": lambda: plan.time_stretch(wave, rate),
            "member": lambda: conv.time_stretch(wave, rate),
            "torch": lambda: torch_route(wave, rate),
        })
        peak_member = peak_above(lambda: conv.time_stretch(wave, rate))
        peak_torch = peak_above(lambda: torch_route(wave, rate))

        def show(name):
            return f"{med[name]:9.3f} ms ({spread[name][0]:.3f} .. {spread[name][1]:.3f})"

        lines += [
            "",
            f"---- rate {rate}: {T} -> {Tout} frames per row",
            f"kernel (rfx_phase_vocoder)          {show('kernel')}   {nbytes / 1e9:.2f} GB read + written, {nbytes / med['kernel'] / 1e6:.0f} GB/s",
            f"copy of the same bytes              {show('copy')}   {nbytes / med['copy'] / 1e6:.0f} GB/s; kernel / copy = {med['kernel'] / med['copy']:.2f}",
            f"Plan.time_stretch                   {show('plan')}",
            f"SpectrogramConverter.time_stretch   {show('member')}   peak allocation {peak_member / 2 ** 30:.2f} GiB",
            f"torch composition                   {show('torch')}   peak allocation {peak_torch / 2 ** 30:.2f} GiB; torch / member = {med['torch'] / med['member']:.2f}",
            f"kernel, ONE row of {T} frames       {show('one row')}   the batch takes {med['kernel'] / B:.3f} ms per row: one row alone is "
            f"{med['one row'] / (med['kernel'] / B):.1f} times that",
        ]
        if med["one row"] > 4 * med["kernel"] / B:
            lines.append(f"    one row is far above the batch's time per row: {fs} threads do not fill the chip and each walks {Tout} steps serially.  The next "
                         "step is a time-split scan - segments of the walk in parallel, each segment's phase offset from a prefix sum of the wrapped "
                         "advances - not built here.")
        del out, src, dst
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
