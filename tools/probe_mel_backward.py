"""
The forward path's backward on the device: what a gradient costs next to the forward call of the same build.

    python tools/probe_mel_backward.py [--runs 9] [--calls 5] [--batch 64] [--out profiles/mel_backward.txt]     (on the GPU)

64 mono rows of 225 351 samples (512 frames each at the default parameters):
* forward alone: `Plan.mel_from_waveform` (rfx_mel_from_waveform, the fused forward kernel);
* forward + backward: that call, then `Plan.mel_from_waveform_backward` (rfx_mel_from_waveform_backward) on a seeded gradient - what one
  step of a mel-domain loss costs;
* the backward's parts that have an entry of their own: `Plan.stft` with the spectrum as its output (the re-analysis),
  `Plan.stft_backward` (weights, frame launch, fold) and `Plan.mel_scale_backward`.
A sample is --calls calls back to back between two events; median of --runs samples after a warm-up of all, the calls alternating.
The launches one by one - the re-analysis, mel_bwd_spec_kernel, the MODE 0 frame launch, mel_bwd_fold_kernel - are told apart by a
kernel trace of this probe (rocprofv3 --kernel-trace --stats -- python tools/probe_mel_backward.py --runs 2); the bytes each of them
moves per frame, which the probe states, turn the trace's durations into achieved rates.  No time is fixed in advance: there is no
earlier figure for a backward; the ratio to the forward call is what is reported.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

SEED, SAMPLES = 7, 225351


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_backward.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    assert torch.cuda.is_available(), "this probe measures on the GPU"

    def event_ms(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.calls

    p = SpectrogramParams()
    plan = _hip.get_plan(p, "cuda")
    B = args.batch
    rng = np.random.default_rng(SEED)
    wave = torch.from_numpy((rng.standard_normal((B, SAMPLES)) * 8000).astype(np.float32)).cuda()
    Tn = plan.lib.rfx_stft_frames(plan.handle, SAMPLES)
    g_mel = torch.randn(B, plan.n_mels, Tn, generator=torch.Generator().manual_seed(SEED)).cuda()
    # the complex gradient of the STFT entry: a few rows are enough to time it per row (a whole batch of it is 2.3 GB)
    Bs = min(B, 8)
    g_spec = plan.stft(wave[:Bs], want_mag=False, want_spec=True)[1]

    def fwd_bwd():
        plan.mel_from_waveform(wave)
        plan.mel_from_waveform_backward(wave, g_mel)

    calls = {
        "forward": lambda: plan.mel_from_waveform(wave),
        "forward+backward": fwd_bwd,
        "backward": lambda: plan.mel_from_waveform_backward(wave, g_mel),
        f"stft ({Bs} rows)": lambda: plan.stft(wave[:Bs], want_mag=False, want_spec=True),
        f"stft_backward ({Bs} rows)": lambda: plan.stft_backward(g_spec, Bs, SAMPLES),
        "mel_scale_backward": lambda: plan.mel_scale_backward(g_mel[:Bs]),
    }
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    samples = {key: [] for key in calls}
    for _ in range(args.runs):
        for key, f in calls.items():
            samples[key].append(event_ms(f))
    ms = {key: statistics.median(v) for key, v in samples.items()}
    spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in samples.items()}

    need = plan.lib.rfx_mel_from_waveform_backward_workspace_bytes(plan.handle, B, SAMPLES)
    one = plan.lib.rfx_mel_from_waveform_backward_workspace_bytes(plan.handle, 1, SAMPLES)
    fs, pitch = plan.frame_stride, 4416 if not plan.generic else 0
    lines = [
        f"---- backward of the forward path: {B} mono rows of {SAMPLES} samples ({Tn} frames each), default parameters; device {torch.cuda.get_device_name(0)}",
        f"time: {args.calls} calls back to back per sample, median of {args.runs} samples after warm-up, events on the stream, the calls alternating "
        "(spread = (max - min) / median)",
        "",
    ]
    for key in calls:
        lines.append(f"{key:28s} {ms[key]:9.3f} ms ({100 * spread[key]:4.1f} %)")
    lines += [
        "",
        f"backward / forward: {ms['backward'] / ms['forward']:.2f}; (forward + backward) / forward: {ms['forward+backward'] / ms['forward']:.2f}; "
        f"{B / ms['forward+backward'] * 1000:.0f} rows per second forward + backward",
        f"workspace of the backward: {need / 2**20:.1f} MiB for {B} rows ({one / 2**20:.1f} MiB for one row: the rows are walked in groups of "
        f"{max(1, (256 << 20) // max(one, 1))})",
        "",
        "bytes per frame each launch of the backward moves (HBM, reads + writes):",
        f"  re-analysis (rfx_stft, spectrum out)   write {fs * 8} (the waveform is read once per ten frames: {p.hop_length * 4})",
        f"  mel_bwd_spec_kernel                    read {fs * 8} spectrum + {plan.n_mels * 4} gradient (strided: {plan.n_mels * 32} in 32-byte sectors), write {fs * 4}",
        f"  frame launch (MODE 0)                  read {fs * 8} + {fs * 4}, write {pitch * 4}",
        f"  mel_bwd_fold_kernel                    read {pitch * 4} (every frame value once from HBM, ten times from cache), write {p.hop_length * 4}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
