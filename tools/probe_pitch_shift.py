"""
Pitch shift: the member, its three stages, the resample kernel against a copy of the bytes it moves, and the torch composition it
replaces.

    python tools/probe_pitch_shift.py [--rows 64] [--frames 512] [--runs 9] [--out profiles/pitch_shift.txt]     (on the GPU)

Workload: `--rows` rows of `--frames` frames at the default parameters (seeded noise of hop * (frames - 1) samples: 5.11 s), shifted
by +1, +2, -5 and +12 semitones.  Every figure is the median of --runs runs after a warm-up of the same shape, device events on the
stream around one call, the routes of a shift alternating.  Recorded, not gated:
    member        SpectrogramConverter.pitch_shift on the device tensor, and Plan.pitch_shift (rfx_pitch_shift) under it.
    stages        Plan.time_stretch; the cut or pad to round(Lw / rate) as a torch copy (the fused entry makes no such pass); the
                  resample kernel alone (rfx_resample_sinc on the stretched rows, table uploaded before).
    resample      bytes: the samples it reads plus the samples it writes, 4 * rows * (L + K) - the table (4 * n * ntaps bytes) stays in
                  cache - over its time; beside it a device-to-device copy that moves the same bytes, and the ratio of the two times.
    torch         the composition a user writes today on the same device tensors: spectrogram_func -> the float32 transcription of
                  torchaudio's phase_vocoder -> waveform_from_spectrogram(length=) -> the dense transcription of
                  torchaudio.functional.resample (tests/resample_oracle.py: conv1d with the (n, 1, 2 width + o) kernel, the kernel built
                  once before the timed calls, as transforms.Resample keeps it) -> cut or pad.  Where the dense float32 kernel would
                  pass --dense-cap-gb the route is not run and the file says so.
    peak          torch.cuda.max_memory_allocated over one call of the member and of the torch route, above what was allocated before.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("riffusion-hobby_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

STEPS = (1, 2, -5, 12)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--dense-cap-gb", type=float, default=1.0, help="largest dense float32 kernel the torch route is run with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_shift.txt"))
    args = ap.parse_args()

    import torch

    import resample_oracle as RO
    import vocoder_oracle as VO
    from riffusion import _hip
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_params import SpectrogramParams

    assert torch.cuda.is_available(), "this probe measures on the GPU"
    p = SpectrogramParams()
    conv = SpectrogramConverter(p, device="cuda")
    plan = conv._plan()
    B, T, sr = args.rows, args.frames, p.sample_rate
    Lw = p.hop_length * (T - 1)
    wave = (torch.randn(B, Lw, generator=torch.Generator().manual_seed(5)) * 8000).cuda()
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

    def fix(y, length):
        L = y.shape[-1]
        return y[..., :length] if length <= L else torch.nn.functional.pad(y, (0, length - L))

    lines = [f"pitch shift on {torch.cuda.get_device_name(0)}: {B} rows of {T} frames ({Lw} samples, {Lw / sr:.2f} s), default parameters; "
             f"medians of {args.runs} runs (min .. max), device events around one call"]
    for n_steps in STEPS:
        rate = 2.0 ** (-float(n_steps) / 12)
        len_stretch, orig = int(round(Lw / rate)), int(sr / rate)
        o, n, _, width = RO.geometry(orig, sr)
        first, taps = _hip.resample_sinc_table(orig, sr, device="cuda")
        ntaps = int(taps.shape[0])
        stretched = plan.time_stretch(wave, rate)
        Ls = int(stretched.shape[1])
        cut = fix(stretched, len_stretch).contiguous()
        K = _hip.resample_sinc_frames(len_stretch, orig, sr)
        out = torch.empty((B, K), dtype=torch.float32, device="cuda")
        nbytes = 4 * B * (len_stretch + K)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        dense_gb = 4.0 * n * (2 * width + o) / 1e9
        dense = RO.dense_kernel(orig, sr, torch.float32, device="cuda")[0] if dense_gb <= args.dense_cap_gb else None

        def kernel():
            _hip.check(plan.lib.rfx_resample_sinc(cut.data_ptr(), B, len_stretch, orig, sr, first.data_ptr(), taps.data_ptr(), ntaps, out.data_ptr(), stream))

        def torch_route(w):
            X = conv.spectrogram_func(w)
            y = conv.waveform_from_spectrogram(VO.phase_vocoder(X, rate, p.hop_length, torch.float32), length=len_stretch)
            return fix(RO.apply_dense(y, orig, sr, dense, width), Lw)

        routes = {
            "member": lambda: conv.pitch_shift(wave, n_steps),
            "plan": lambda: plan.pitch_shift(wave, n_steps),
            "stretch": lambda: plan.time_stretch(wave, rate),
            "cut": lambda: fix(stretched, len_stretch).contiguous(),
            "kernel": kernel,
            "copy": lambda: dst.copy_(src),
        }
        if dense is not None:
            routes["torch"] = lambda: torch_route(wave)
        med, spread = medians(routes)
        peak_member = peak_above(lambda: conv.pitch_shift(wave, n_steps))
        peak_torch = peak_above(lambda: torch_route(wave)) if dense is not None else 0

        def show(name):
            return f"{med[name]:9.3f} ms ({spread[name][0]:.3f} .. {spread[name][1]:.3f})"

        lines += [
            "",
            f"---- {n_steps:+d} semitones: rate {rate:.5f}, stretched rows {Ls} -> cut or padded to {len_stretch}, resampled {orig} -> {sr} = {o} / {n}, "
            f"{ntaps} taps, table {4 * n * ntaps / 2 ** 20:.2f} MiB, K = {K}",
            f"SpectrogramConverter.pitch_shift     {show('member')}   peak allocation {peak_member / 2 ** 30:.2f} GiB",
            f"Plan.pitch_shift (rfx_pitch_shift)   {show('plan')}",
            f"  stage 1, Plan.time_stretch         {show('stretch')}",
            f"  stage 2, cut or pad as a copy      {show('cut')}   (not a pass of the fused entry)",
            f"  stage 3, rfx_resample_sinc         {show('kernel')}   {nbytes / 1e6:.0f} MB read + written, {nbytes / med['kernel'] / 1e6:.0f} GB/s",
            f"  copy of the same bytes             {show('copy')}   {nbytes / med['copy'] / 1e6:.0f} GB/s; kernel / copy = {med['kernel'] / med['copy']:.2f}",
        ]
        if dense is not None:
            lines.append(f"torch composition                    {show('torch')}   dense kernel {dense_gb:.3f} GB, peak allocation {peak_torch / 2 ** 30:.2f} GiB; "
                         f"torch / member = {med['torch'] / med['member']:.2f}")
        else:
            lines.append(f"torch composition                    not run: the dense float32 kernel ({n} x {2 * width + o}) would take {dense_gb:.1f} GB, "
                         f"above --dense-cap-gb {args.dense_cap_gb:g}")
        del out, src, dst, dense, cut, stretched
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
