"""Bytes of every decode variant through every Python entry, for comparing two versions of the `riffusion` package on one library.

    python tools/probe_decode_variants.py [--package DIR] > one.txt      one line per (entry, variant): label, SHA-256 of the output
    python tools/probe_decode_variants.py --compare parent.txt this.txt  the table of profiles/decode_variant_refactor.txt

--package DIR: the directory that holds the `riffusion` package to import (default: this tree's); run one fresh process per
package, both with RFX_LIB_PATH naming the same librfx.so.  Inputs are host-seeded (numpy default_rng), 5 tiles of width 48, 2
Griffin-Lim iterations, seed 11; the variants are those of tests/test_gpu_decode_variants.py."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, ITERS, SEED = 5, 48, 2, 11


def sha(x) -> str:
    import numpy as np
    import torch

    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:32]


def probe() -> None:
    import numpy as np
    import torch

    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams
    from riffusion.util import audio_util

    print(f"riffusion package: {os.path.dirname(audio_util.__file__)}", file=sys.stderr)
    rng = np.random.default_rng(20240)
    tiles = rng.integers(0, 256, size=(N, 512, W, 3), dtype=np.uint8)
    guides = (rng.standard_normal((N, 1, 21000)) * 3000).astype(np.float32)
    mask = rng.random((N, 512, W)) < 0.5
    mask[:, :, :5] = True
    # (what the batch entry calls it, the torch-level seam, the single-image entry)
    names = {"guide": ("guide_waveforms", "guide", "guide_segment")}
    variants = {"plain": {}, "lstsq": dict(inverse_mel="lstsq"), "guided": dict(guide=True), "guided + hold_frames": dict(guide=True, hold_frames=(3, 2)),
                "guided + band mask": dict(guide=True, hold_mask=True), "loop": dict(loop=True), "loop + guided": dict(loop=True, guide=True),
                "peaks": dict(phase_start="peaks")}
    for stereo in (False, True):
        conv = SpectrogramImageConverter(SpectrogramParams(stereo=stereo), device="cuda")
        C = 2 if stereo else 1
        ch = "stereo" if stereo else "mono"
        mel = torch.from_numpy((rng.random((N * C, 512, W)) ** 4 * 3e6).astype(np.float32))
        for name, v in variants.items():
            loop = bool(v.get("loop"))

            def kw(which: int, n: slice = slice(None)) -> dict:
                out = {k: x for k, x in v.items() if k not in ("guide", "hold_mask")}
                if v.get("guide"):
                    g = guides[n]
                    if which == 1:  # one guide row per mel row
                        g = torch.from_numpy(np.repeat(g[:, 0], C, axis=0))
                    elif which == 2:
                        g = audio_util.PcmSegment(np.clip(g[0], -32768, 32767).astype(np.int16).T.copy(), conv.p.sample_rate)
                    out[names["guide"][which]] = g
                if v.get("hold_mask"):
                    out["hold_mask"] = np.repeat(mask[n], C, axis=0) if which == 1 else mask[0] if which == 2 else mask[n]
                return out

            batch = dict(kw(0), seed=SEED, griffin_lim_iters=ITERS, tiles_per_call=2)
            print(f"{ch} images pcm | {name} | {sha(conv.audio_from_spectrogram_images(tiles, **batch))}")
            print(f"{ch} images waveform | {name} | {sha(conv.audio_from_spectrogram_images(tiles, return_waveform=True, **batch))}")
            pcm, err = conv.audio_from_spectrogram_images(tiles, **{"return_loop_error" if loop else "return_error": True}, **batch)
            print(f"{ch} images error route pcm | {name} | {sha(pcm)}")
            print(f"{ch} images error route errors | {name} | {sha(err)}")
            wave = conv.converter.waveform_from_mel_amplitudes(mel, seed=SEED, channels_per_clip=C, griffin_lim_iters=ITERS, **kw(1))
            print(f"{ch} waveform_from_mel_amplitudes | {name} | {sha(wave)}")
            torch.manual_seed(SEED)
            seg = conv.audio_from_spectrogram_image(tiles[0], griffin_lim_iters=ITERS, **kw(2, slice(0, 1)))
            print(f"{ch} audio_from_spectrogram_image | {name} | {sha(seg.get_array_of_samples())}")


def compare(parent: str, this: str) -> int:
    def read(path: str) -> dict:
        with open(path) as f:
            return dict(line.rsplit(" | ", 1) for line in f.read().splitlines() if " | " in line)

    a, b = read(parent), read(this)
    width = max(len(k) for k in a)
    print(f"{'entry | variant'.ljust(width)} {'parent'.ljust(32)} this change")
    unequal = 0
    for k in a:
        same = a[k] == b.get(k)
        unequal += not same
        print(f"{k.ljust(width)} {a[k]} {b.get(k, 'missing'.ljust(32))} {'equal' if same else 'UNEQUAL'}")
    missing = [k for k in b if k not in a]
    print(f"{len(a)} / {len(a)} entries, {unequal} unequal" + (f", {len(missing)} only in this change" if missing else ""))
    return 1 if unequal or missing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package", default=os.path.join(ROOT, "riffusion-hobby_amd"))
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.package))
    probe()
