"""
Tiles from JPEG files that are in host memory: the parent's route (Pillow `Image.open` + `image_util.rgb_array_from_image` file by
file on one thread, as the batch CLI runs it, `np.stack`, upload) against SpectrogramImageConverter.images_from_jpeg_bytes (parse
the headers, upload the coded bytes, decode on the device), in one run on one box, both ending in an (N, H, W, 3) uint8 tensor
on the device - the same pixels.

    python tools/probe_jpeg_decode.py [--runs 9] [--out profiles/jpeg_decode.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/probe_jpeg_decode.py --kernels-only     (the per-kernel split)

Workloads, 64 files of 512 x 512 at quality 75 each: the og_beat golden tile 64 times, and 64 uniform-noise tiles
(helpers.synthetic_tiles_u8: the longest scans a tile gets).  Host-clock times of runs that end in a device synchronise, the two
routes alternating, after one warm-up each; median and the range of the runs.  The subsequence size and the rounds the scans take
to synchronise come from the host emulator (tests/emu/rfx_jpeg_dec_emu.cpp), which runs the kernel's scheme.
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import synthetic_tiles_u8  # noqa: E402
from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import image_util  # noqa: E402


def jpeg(tile):
    buf = io.BytesIO()
    Image.fromarray(tile).save(buf, "JPEG", quality=75)
    return buf.getvalue()


def pillow_route(files, device):
    t0 = time.perf_counter()
    tiles = []
    for f in files:
        with Image.open(io.BytesIO(f)) as im:
            tiles.append(image_util.rgb_array_from_image(im))
    t1 = time.perf_counter()
    out = torch.from_numpy(np.stack(tiles)).to(device)
    torch.cuda.synchronize()
    return out, t1 - t0, time.perf_counter() - t1


def device_route(conv, files):
    t0 = time.perf_counter()
    out, _ = conv.images_from_jpeg_bytes(files, return_device=True, tiles_per_call=len(files))
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def device_stages(conv, files):
    """(seconds of the header parse, of Plan.jpeg_decode: upload, kernels and the read of the status)"""
    plan = conv.converter._plan()
    t0 = time.perf_counter()
    infos = [image_util.jpeg_parse(f) for f in files]
    t1 = time.perf_counter()
    plan.jpeg_decode([f[i.scan[0]:i.scan[1]] for f, i in zip(files, infos)], infos[0].height, infos[0].width,
                     np.stack([i.qtables for i in infos]), np.stack([i.huffman for i in infos]))
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1


def emulator_rounds(files):
    from jpeg_decode_cases import _emu, emu_decode

    stats = np.array([emu_decode(f)[2] for f in files])
    return _emu().emu_jpeg_dec_sub_bits(), _emu().emu_jpeg_dec_group(), stats


def spread(values):
    v = [x * 1e3 for x in values]
    return f"{statistics.median(v):8.2f} ms (runs {min(v):.2f} .. {max(v):.2f})"


def measure(label, conv, files, runs, lines):
    plan = conv.converter._plan()
    want, _, _ = pillow_route(files, plan.device)  # warm-up, and the pixels to hold the device route to
    got, _ = device_route(conv, files)
    assert torch.equal(got, want), "the two routes disagree"
    a, b, stages = [], [], []
    for _ in range(runs):  # alternating
        a.append(pillow_route(files, plan.device)[1:])
        b.append(device_route(conv, files)[1])
        stages.append(device_stages(conv, files))
    a_total, b_total = [x + y for x, y in a], b
    ratios = sorted(x / y for x, y in zip(a_total, b_total))
    s_bits, group, stats = emulator_rounds(files[:1] if len(set(files)) == 1 else files)
    n = len(files)
    lines += [
        f"{label}: {n} files of {want.shape[1]} x {want.shape[2]}, {sum(map(len, files)) / 1e6:.2f} MB of JPEG -> {want.numel() / 1e6:.1f} MB of RGB on the device",
        f"  (a) Pillow open loop + np.stack + upload: {spread(a_total)}   (loop {spread(x for x, _ in a)} = "
        f"{statistics.median(x for x, _ in a) * 1e3 / n:.3f} ms per file; stack + upload {spread(y for _, y in a)})",
        f"  (b) images_from_jpeg_bytes:               {spread(b_total)}   ({statistics.median(ratios):.1f}x, runs {ratios[0]:.1f}x .. {ratios[-1]:.1f}x; "
        f"{n / statistics.median(b_total):.0f} files/s)",
        f"      of (b): header parse {spread(s[0] for s in stages)}   upload + kernels + status read {spread(s[1] for s in stages)}",
        f"      subsequences of {s_bits} bits, {group} to a group: {stats[:, 1].min()} .. {stats[:, 1].max()} per scan in {stats[:, 2].min()} .. {stats[:, 2].max()} "
        f"groups; rounds to synchronise a group: most {stats[:, 0].max()}, per scan (summed over its groups) median {int(np.median(stats[:, 3]))}, most {stats[:, 3].max()}",
    ]
    return statistics.median(a_total), statistics.median(b_total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="only the device route, three times per workload: for a kernel trace")
    args = ap.parse_args()
    assert args.runs >= 5
    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False), device="cuda")
    og = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "og_beat.png")).convert("RGB"))
    workloads = [("og_beat x 64", [jpeg(og)] * 64), ("uniform noise", [jpeg(t) for t in synthetic_tiles_u8(64)])]
    if args.kernels_only:
        for _, files in workloads:
            for _ in range(3):
                device_route(conv, files)
        return
    lines = [f"(N, H, W, 3) tiles on the device from JPEG files (quality 75, Pillow's defaults) in host memory; device {torch.cuda.get_device_name(0)}, "
             f"Pillow {Image.__version__}, {args.runs} alternating runs after warm-up, host clock to a device synchronise; same pixels on both routes"]
    results = [measure(label, conv, files, args.runs, lines) for label, files in workloads]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    assert all(b < a for a, b in results), "the device route is not faster than the Pillow route on every set"


if __name__ == "__main__":
    main()
