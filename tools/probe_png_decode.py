"""
Tiles from PNG files that are in host memory, three routes in one run on one box, all ending in an (N, H, W, 3) uint8 tensor on the
device - the same pixels: (a) the batch CLI's default (Pillow `Image.open` + `image_util.rgb_array_from_image` file by file on one
thread, `np.stack`, upload); (b) the same loop in a pool of 16 threads (Pillow releases the GIL while it decodes); (c)
SpectrogramImageConverter.images_from_png_bytes (walk the chunks, upload the IDAT bytes, inflate and unfilter on the device).

    python tools/probe_png_decode.py [--runs 9] [--out profiles/png_decode.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/probe_png_decode.py --kernels-only     (the per-kernel split)

Workloads, 64 files of 512 x 512 each: the five golden seed tiles in turn, saved by Pillow's default `save` as RGB (what the
reference writes), and the same tiles written grey by `png_bytes_from_images(mode="auto")`.  Host-clock times of runs that end in a
device synchronise, the routes alternating, after one warm-up each; medians and the range of the runs.
"""
import argparse
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import image_util  # noqa: E402

SEEDS = ("agile.png", "marim.png", "motorway.png", "og_beat.png", "vibes.png")
POOL = 16


def open_one(f):
    with Image.open(io.BytesIO(f)) as im:
        return image_util.rgb_array_from_image(im)


def pillow_route(files, device, pool=None):
    t0 = time.perf_counter()
    tiles = list(pool.map(open_one, files)) if pool else [open_one(f) for f in files]
    t1 = time.perf_counter()
    out = torch.from_numpy(np.stack(tiles)).to(device)
    torch.cuda.synchronize()
    return out, t1 - t0, time.perf_counter() - t1


def device_route(conv, files):
    t0 = time.perf_counter()
    out, _ = conv.images_from_png_bytes(files, return_device=True, tiles_per_call=len(files))
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def device_stages(conv, files):
    """(seconds of the chunk walk and the join of the IDAT payloads, of Plan.png_decode: upload, kernels and the read of the status)"""
    plan = conv.converter._plan()
    t0 = time.perf_counter()
    infos = [image_util.png_parse(f) for f in files]
    streams = [b"".join(f[a:b] for a, b in i.idat) for f, i in zip(files, infos)]
    t1 = time.perf_counter()
    plan.png_decode(streams, infos[0].height, infos[0].width, infos[0].color_type)
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1


def spread(values):
    v = [x * 1e3 for x in values]
    return f"median {statistics.median(v):8.2f} ms (runs {min(v):.2f} .. {max(v):.2f})"


def measure(label, conv, files, runs, lines, pool):
    plan = conv.converter._plan()
    want, _, _ = pillow_route(files, plan.device)  # warm-up, and the pixels to hold the other routes to
    assert torch.equal(pillow_route(files, plan.device, pool)[0], want) and torch.equal(device_route(conv, files)[0], want), "the routes disagree"
    a, b, c, stages = [], [], [], []
    for _ in range(runs):  # alternating
        a.append(pillow_route(files, plan.device)[1:])
        b.append(pillow_route(files, plan.device, pool)[1:])
        c.append(device_route(conv, files)[1])
        stages.append(device_stages(conv, files))
    a_total, b_total = [x + y for x, y in a], [x + y for x, y in b]
    n = len(files)
    lines += [
        f"{label}: {n} files of {want.shape[1]} x {want.shape[2]}, {sum(map(len, files)) / 1e6:.2f} MB of PNG -> {want.numel() / 1e6:.1f} MB of RGB on the device",
        f"  (a) Pillow open loop + np.stack + upload:       {spread(a_total)}   (loop {spread(x for x, _ in a)}; stack + upload {spread(y for _, y in a)})",
        f"  (b) the loop in a pool of {POOL} threads + upload: {spread(b_total)}   (pool {spread(x for x, _ in b)})",
        f"  (c) images_from_png_bytes:                      {spread(c)}   ({n / statistics.median(c):.0f} files/s; (a) / (c) {statistics.median(a_total) / statistics.median(c):.2f}, "
        f"(b) / (c) {statistics.median(b_total) / statistics.median(c):.2f})",
        f"      of (c): chunk walk and IDAT join {spread(s[0] for s in stages)}   upload + kernels + status read {spread(s[1] for s in stages)}",
    ]


def workloads(conv):
    seeds = [np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", s)).convert("RGB")) for s in SEEDS]
    rgb = []
    for t in seeds:
        buf = io.BytesIO()
        Image.fromarray(t).save(buf, "PNG")
        rgb.append(buf.getvalue())
    grey = conv.png_bytes_from_images(np.stack(seeds), mode="auto")
    pick = [i % len(SEEDS) for i in range(64)]
    return [("seed tiles, Pillow's default save as RGB", [rgb[i] for i in pick]), ("the same tiles, png_bytes_from_images(mode='auto')", [grey[i] for i in pick])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="only the device route, three times per workload: for a kernel trace")
    args = ap.parse_args()
    assert args.runs >= 5
    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False), device="cuda")
    sets = workloads(conv)
    if args.kernels_only:
        for _, files in sets:
            for _ in range(3):
                device_route(conv, files)
        return
    lines = [f"(N, H, W, 3) tiles on the device from PNG files in host memory; device {torch.cuda.get_device_name(0)}, Pillow {Image.__version__}, "
             f"{args.runs} alternating runs after warm-up, host clock to a device synchronise; same pixels on all routes; every figure a median"]
    with ThreadPoolExecutor(POOL) as pool:
        for label, files in sets:
            measure(label, conv, files, args.runs, lines, pool)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
