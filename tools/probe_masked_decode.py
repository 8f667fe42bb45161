"""
Masked decode against the start-only guided decode: time of the product entry point, reconstruction error and how far the kept bins
stay from the source, by iteration count.

    python tools/probe_masked_decode.py [--tiles 64] [--runs 9] [--out profiles/masked_decode.txt]     (on the GPU)

Workload: that of tools/probe_guided_decode.py and tools/probe_held_decode.py - `--tiles` mono 512-frame clips cut from the three
golden recordings, encoded to tiles on the device, the clips themselves as the guides - with the reference's stock mask
tests/golden/mask_gradient_dark.png (a frequency mask: 30.7 % of the tile kept, its dark top rows) as `hold_mask`.  For n_iter in
0, 2, 4, 8, 32, `audio_from_spectrogram_images` (tiles, guides and mask on the device, result left there, all tiles in one call) is
timed - median of --runs runs after a warm-up, events on the stream, the forms alternating - as
    guided        guide_waveforms only: the start-only guided call, on the run form;
    guided frames hold_frames=(0, 0): the same bytes on the per-frame form, the form a masked call takes;
    masked        hold_mask=the mask;
one further call each with return_error=True gives the mean spectral convergence of the clips (against the tiles' magnitudes), and
one with return_waveform=True the kept-bin fidelity: 10 log10 of sum |G|^2 over sum |G - X|^2 on the held bins, G the guide's STFT
and X the output's, pooled over the clips.

Expected from the derivation, not gated: over `guided frames`, one launch of the first launch's class, two streaming
passes over the magnitudes and one more read of B x L floats per fold; nothing at n_iter = 0.  A mask removes no iteration work.
The figures to compare with are the parent commit's in profiles/guided_decode.txt and profiles/held_decode.txt.
"""
import argparse
import glob
import os
import statistics
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

ITERS = (0, 2, 4, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image

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

    def golden_clips(n: int, samples: int) -> np.ndarray:
        """(n, 1, samples) float32 at int16 scale"""
        tracks = []
        for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "clip_*.wav"))):
            with wave.open(path) as w:
                assert w.getframerate() == 44100 and w.getsampwidth() == 2
                pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
            tracks.append(pcm.astype(np.float32).mean(axis=1))
        clips, k = [], 0
        while len(clips) < n:
            track, start = tracks[k % len(tracks)], 1000 * (k // len(tracks))
            assert start + samples <= len(track), "the golden recordings hold no more clips of this length"
            clips.append(track[start:start + samples])
            k += 1
        return np.stack(clips)[:, None, :]

    N, T = args.tiles, 512
    p = SpectrogramParams()
    conv = SpectrogramImageConverter(p, device="cuda")
    plan = conv.converter._plan()
    clips = torch.from_numpy(golden_clips(N, p.hop_length * (T - 1))).cuda()
    tiles, _ = conv.spectrogram_images_from_waveforms(clips, return_device=True)
    assert tuple(tiles.shape) == (N, 512, T, 3)
    bands = image_util.hold_mask_from_image(Image.open(os.path.join(ROOT, "tests", "golden", "mask_gradient_dark.png")))
    assert bands.shape == (512, T)
    mask = torch.from_numpy(bands).cuda()[None].expand(N, 512, T).contiguous()
    forms = {"guided": dict(), "guided frames": dict(hold_frames=(0, 0)), "masked": dict(hold_mask=mask)}

    # the held bins of a clip (n_stft, T) bool, from the bit mask the call itself uses
    words = plan.hold_bins_from_bands(mask[:1].to(torch.uint8))[0]  # (T, words) int32
    held = (((words[:, :, None] >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1) != 0).reshape(T, -1)[:, :plan.n_stft].t().contiguous()
    kept_share = float(held.float().mean())

    def decode(n_iter: int, form: str, **kw):
        return conv.audio_from_spectrogram_images(tiles, seed=7, tiles_per_call=N, return_device=True, guide_waveforms=clips, griffin_lim_iters=n_iter,
                                                  **forms[form], **kw)

    def spectrum(rows: torch.Tensor) -> torch.Tensor:
        _, spec, Tn = plan.stft(rows.contiguous(), want_mag=False, want_spec=True)
        return plan.unpack_complex(spec, rows.shape[0], Tn)

    def fidelity_db(wave_out: torch.Tensor) -> float:
        """kept-bin fidelity pooled over the clips, a clip at a time (a clip's spectrum is 36 MB)"""
        num = den = 0.0
        for i in range(N):
            G, X = spectrum(clips[i]).to(torch.complex128)[0], spectrum(wave_out[i]).to(torch.complex128)[0]
            num += float(G[held].abs().pow(2).sum())
            den += float((G[held] - X[held]).abs().pow(2).sum())
        return 10.0 * float(np.log10(num / den))

    times, sc, fid = {}, {}, {}
    for n in ITERS:
        for f in forms:
            decode(n, f)
        torch.cuda.synchronize()
        samples = {f: [] for f in forms}
        for _ in range(args.runs):
            for f in forms:
                samples[f].append(event_ms(lambda: decode(n, f)))
        for f in forms:
            times[(n, f)] = (statistics.median(samples[f]), (max(samples[f]) - min(samples[f])) / statistics.median(samples[f]))
            sc[(n, f)] = float(decode(n, f, return_error=True)[1].mean())
            if f != "guided frames":
                fid[(n, f)] = fidelity_db(decode(n, f, return_waveform=True))
    same0 = torch.equal(decode(0, "guided"), decode(0, "masked"))
    same_forms = all(torch.equal(decode(n, "guided"), decode(n, "guided frames")) for n in ITERS)

    lines = [
        f"---- masked decode of {N} mono tiles of {T} frames cut from the golden recordings, the clips themselves as guides, hold_mask = "
        f"tests/golden/mask_gradient_dark.png ({100 * bands.mean():.1f} % of the tile kept, {100 * kept_share:.1f} % of the linear bins held); default "
        f"parameters (InverseMelScale 200 steps); device {torch.cuda.get_device_name(0)}",
        f"audio_from_spectrogram_images, all tiles in one call, device in / device out; median of {args.runs} runs after warm-up, events on the stream, the "
        "three forms alternating; SC = mean spectral convergence of the clips (return_error=True); fidelity = kept-bin fidelity in dB, pooled over the clips",
        "`guided` is the start-only guided call (run form), `guided frames` the same bytes on the per-frame form (hold_frames=(0, 0)), `masked` the masked call "
        "(per-frame form)",
        "",
        "n_iter   guided ms (spread)     SC    fidelity | guided frames ms (spread)  vs guided    SC    | masked ms (spread)  vs guided  vs guided frames    SC    fidelity",
    ]
    for n in ITERS:
        tg, tf = times[(n, "guided")][0], times[(n, "guided frames")][0]
        t, s = times[(n, "masked")]
        lines.append(f"{n:6d}   {tg:9.3f} ({100 * times[(n, 'guided')][1]:4.1f} %)  {sc[(n, 'guided')]:.4f}  {fid[(n, 'guided')]:6.1f}  "
                     f" |     {tf:9.3f} ({100 * times[(n, 'guided frames')][1]:4.1f} %)      {100 * (tf / tg - 1):+6.1f} %   {sc[(n, 'guided frames')]:.4f}  "
                     f"| {t:9.3f} ({100 * s:4.1f} %)  {100 * (t / tg - 1):+6.1f} %   {100 * (t / tf - 1):+6.1f} %         {sc[(n, 'masked')]:.4f}  {fid[(n, 'masked')]:6.1f}")
    t32 = {f: times[(32, f)][0] for f in forms}
    lines += [
        "",
        f"n_iter = 0: the masked call gives the bytes of the guided call: {'yes' if same0 else 'NO'}; `guided frames` gives the bytes of `guided` at every "
        f"n_iter: {'yes' if same_forms else 'NO'}",
        f"over the per-frame form a mask costs {t32['masked'] - t32['guided frames']:+.2f} ms of the whole decode at 32 iterations "
        f"({100 * (t32['masked'] / t32['guided frames'] - 1):+.1f} %): the c launch, the two splits and the folds' extra read; over the run form "
        f"{100 * (t32['masked'] / t32['guided'] - 1):+.1f} %, the per-frame form's premium included",
        f"kept-bin fidelity at 32 iterations: start-only {fid[(32, 'guided')]:.1f} dB, masked {fid[(32, 'masked')]:.1f} dB (at n_iter = 0 both "
        f"{fid[(0, 'guided')]:.1f} dB); spectral convergence {sc[(32, 'guided')]:.4f} against {sc[(32, 'masked')]:.4f}: the trade the mask makes",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
