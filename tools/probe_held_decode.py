"""
Held frames against the start-only guided decode: time of the product entry point and reconstruction error, by iteration count
and by the share of the frames that is held.

    python tools/probe_held_decode.py [--tiles 64] [--runs 9] [--out profiles/held_decode.txt]     (on the GPU)
    python tools/probe_held_decode.py --resources [--out profiles/held_decode.txt]                  (no GPU: reads the compiler's report)

Workload: that of tools/probe_guided_decode.py - `--tiles` mono 512-frame clips cut from the three golden recordings, encoded to
tiles on the device, the clips themselves as the guides.  For n_iter in 4, 8, 32, `audio_from_spectrogram_images` (tiles and guides on
the device, result left there, all tiles in one call) is timed - median of --runs runs after a warm-up, events on the stream, the
forms alternating - as
    guided        guide_waveforms only: the start-only guided call.  Its kernels and its host path are the parent commit's (the
                  unlisted instantiations compile to the same instructions as before held frames existed), on the run form;
    hold none     hold_frames=(0, 0): same bytes as `guided`, but a held call - the per-frame form, the list of all frames;
    hold half     hold_frames=(128, 128): half of the frames held;
    hold all      hold_frames=(512, 0): every frame held - launches 1 .. n_iter run only their folds;
and one further call each with return_error=True gives the mean spectral convergence of the clips.

Expected, not gated: `hold none` pays the per-frame form's premium over runs (profiles/r06_griffinlim_forms_by_batch.txt: about 29 %
of the Griffin-Lim time at 32 tiles), and the cost falls roughly linearly with the held share.

--resources: registers and scratch of the list-walking kernels beside their unlisted twins, from the ISA hipcc emits for gfx950
(tools/isa_resources.py).  The sections of the file are kept apart by their headings; either run keeps the other's, and the
hand-written one on bench.py.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ITERS = (4, 8, 32)
TIMES_MARKER = "---- time and reconstruction error"
RES_MARKER = "---- registers and scratch"
NOTES_MARKER = "---- bench.py and the unheld paths"  # kept by hand: what no run of this tool measures
MARKERS = (TIMES_MARKER, RES_MARKER, NOTES_MARKER)


def sections(path):
    """{marker: text} of an existing file"""
    out = {}
    if os.path.exists(path):
        text = open(path).read()
        marks = sorted((text.index(m), m) for m in MARKERS if m in text)
        for i, (at, m) in enumerate(marks):
            out[m] = text[at:marks[i + 1][0] if i + 1 < len(marks) else len(text)].rstrip("\n") + "\n"
    return out


def write(path, new):
    have = sections(path)
    have.update(new)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(have[m] for m in MARKERS if m in have))


def resources():
    from concurrent.futures import ThreadPoolExecutor

    import isa_resources

    files = ("rfx_gl.hip", "rfx_fam.hip", "rfx_fam_pk.hip", "rfx_generic.hip", "rfx_czt.hip", "rfx_czt_list.hip")
    with ThreadPoolExecutor(len(files)) as ex:
        rows = [r for rs in ex.map(lambda f: isa_resources.kernels_of(os.path.join(isa_resources.CSRC, f)), files) for r in rs]
    by_name = {r["kernel"].split("(")[0].replace("void rfx::", ""): r for r in rows}
    lines = [RES_MARKER + " of the list-walking kernels beside their unlisted twins (hipcc's report for gfx950, tools/isa_resources.py)",
             "kernel                                     VGPRs  scratch B  scratch instr. |  unlisted twin: VGPRs  scratch B  scratch instr. | same occupancy class"]
    differ = []
    for name, r in sorted(by_name.items()):
        if "_list_kernel" not in name:
            continue
        t = by_name[name.replace("_list_kernel", "_kernel")]
        # waves per SIMD follow the VGPR count in steps of 8 registers up to 512 / waves
        same = (512 // ((r["vgpr"] + 7) // 8 * 8)) == (512 // ((t["vgpr"] + 7) // 8 * 8))
        if (r["vgpr"], r["scratch_bytes"]) != (t["vgpr"], t["scratch_bytes"]):
            differ.append(name)
        lines.append(f"{name:42s} {r['vgpr']:5d}  {r['scratch_bytes']:9d}  {r['scratch_instructions_static']:14d} |  {t['vgpr']:20d}  {t['scratch_bytes']:9d}  "
                     f"{t['scratch_instructions_static']:14d} | {'yes' if same else 'NO'}")
    lines.append("")
    lines.append("same registers and scratch as the twin: " + ("every kernel" if not differ else "all but " + ", ".join(differ) +
                                                                " (a few registers either way: one more loop-carried value, the list pointer, "
                                                                "and another allocation)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    return {RES_MARKER: text}


def timings(args):
    import glob
    import wave

    import numpy as np
    import torch

    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

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
    clips = torch.from_numpy(golden_clips(N, p.hop_length * (T - 1))).cuda()
    tiles, _ = conv.spectrogram_images_from_waveforms(clips, return_device=True)
    assert tuple(tiles.shape) == (N, 512, T, 3)
    forms = {"guided": None, "hold none": (0, 0), "hold half": (T // 4, T // 4), "hold all": (T, 0)}

    def decode(n_iter: int, form: str, error: bool = False):
        return conv.audio_from_spectrogram_images(tiles, seed=7, tiles_per_call=N, return_device=True, return_error=error, guide_waveforms=clips,
                                                  griffin_lim_iters=n_iter, hold_frames=forms[form])

    times, sc = {}, {}
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
            sc[(n, f)] = float(decode(n, f, True)[1].mean())
    same = all(torch.equal(decode(n, "guided"), decode(n, "hold none")) for n in ITERS)

    lines = [
        TIMES_MARKER + f": held decode of {N} mono tiles of {T} frames cut from the golden recordings, the clips themselves as guides; default "
        f"parameters (InverseMelScale 200 steps); device {torch.cuda.get_device_name(0)}",
        f"audio_from_spectrogram_images, all tiles in one call, device in / device out; median of {args.runs} runs after warm-up, events on the "
        "stream, the four forms alternating; SC = mean spectral convergence of the clips (return_error=True)",
        "`guided` is the start-only guided call: the parent commit's kernels and host path (run form); the three others are held calls (per-frame form)",
        "",
        "n_iter   guided ms (spread)     SC    | hold none ms (spread)  vs guided    SC    | hold half ms (spread)  vs guided    SC    | hold all ms (spread)  vs guided    SC",
    ]
    for n in ITERS:
        tg = times[(n, "guided")][0]
        row = f"{n:6d}   {tg:9.3f} ({100 * times[(n, 'guided')][1]:4.1f} %)  {sc[(n, 'guided')]:.4f}"
        for f in ("hold none", "hold half", "hold all"):
            t, s = times[(n, f)]
            row += f"  | {t:9.3f} ({100 * s:4.1f} %)  {100 * (t / tg - 1):+6.1f} %   {sc[(n, f)]:.4f}"
        lines.append(row)
    t32 = {f: times[(32, f)][0] for f in forms}
    lines += [
        "",
        f"`hold none` gives the bytes of `guided`: {'yes' if same else 'NO'}",
        f"the headline at no hold is the per-frame form's premium over runs: {100 * (t32['hold none'] / t32['guided'] - 1):+.1f} % of the whole decode at 32 "
        "iterations (the InverseMelScale SGD and the codecs are in both); making the run kernel hold-aware would remove it and is not part of this",
        f"per held half of the frames the decode at 32 iterations falls by {t32['hold none'] - t32['hold half']:.2f} ms, per the other half by "
        f"{t32['hold half'] - t32['hold all']:.2f} ms (linear in the held share if the two are equal); a held decode is cheaper than the start-only one "
        f"from a held share of about {100 * (t32['hold none'] - t32['guided']) / max(t32['hold none'] - t32['hold all'], 1e-9):.0f} % on",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    return {TIMES_MARKER: text}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_decode.txt"))
    args = ap.parse_args()
    write(args.out, resources() if args.resources else timings(args))


if __name__ == "__main__":
    main()
