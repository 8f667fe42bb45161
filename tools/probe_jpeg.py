"""
JPEG files from tiles that are on the device: the parent's route (download the RGB bytes, Pillow `save` into BytesIO tile by
tile) against SpectrogramImageConverter.jpeg_bytes_from_images (encode on the device, download the coded bytes), in one run on one
box, both ending in host `bytes` - the same bytes.

    python tools/probe_jpeg.py [--runs 7] [--out profiles/jpeg_encode.txt]

Workloads: 64 tiles of 512 x 512 (helpers.synthetic_tiles_u8: noise, the longest scans a tile gets) without EXIF, and the 49
mono tiles of tools/probe_encode_clips.py's 240 s track with their EXIF.  Host-clock medians of --runs runs after one warm-up;
the device route's stages are timed with events on the stream.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import synthetic_tiles_u8  # noqa: E402
from probe_encode_clips import make_track  # noqa: E402
from riffusion import _hip  # noqa: E402
from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402
from riffusion.util import audio_util  # noqa: E402


def pillow_route(tiles_d, exifs):
    """(files, seconds of the download, seconds of the save loop)"""
    t0 = time.perf_counter()
    host = tiles_d.cpu().numpy()
    t1 = time.perf_counter()
    files = []
    for tile, exif in zip(host, exifs):
        buf = io.BytesIO()
        Image.fromarray(tile).save(buf, format="JPEG", **({} if exif is None else {"exif": exif}))
        files.append(buf.getvalue())
    return files, t1 - t0, time.perf_counter() - t1


def device_route(conv, tiles_d, exifs):
    t0 = time.perf_counter()
    files = conv.jpeg_bytes_from_images(tiles_d, exif=None if exifs[0] is None else exifs)
    return files, time.perf_counter() - t0


def device_stages(plan, tiles_d):
    """rfx_jpeg_encode_u8, the read of the sizes, the gather of the used bytes, their download (ms, events)"""
    N, H, W, _ = tiles_d.shape
    lib = plan.lib
    cap, need = lib.rfx_jpeg_scan_capacity(H, W), lib.rfx_jpeg_encode_workspace_bytes(N, H, W)
    qt = plan.device_constant(("jpeg_qtables", 75), lambda: _hip.jpeg_quant_tables(75).view(np.int16))
    scan = torch.empty((N, cap), dtype=torch.uint8, device=plan.device)
    ws = torch.empty(need, dtype=torch.uint8, device=plan.device)
    sizes_d = torch.empty(N, dtype=torch.int32, device=plan.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    _hip.check(lib.rfx_jpeg_encode_u8(tiles_d.data_ptr(), N, H, W, qt.data_ptr(), scan.data_ptr(), sizes_d.data_ptr(), ws.data_ptr(),
                                      _hip.current_stream(plan.device)))
    ev[1].record()
    sizes = [int(v) for v in sizes_d.cpu()]
    ev[2].record()
    packed = torch.cat([scan[n, :s] for n, s in enumerate(sizes)])
    ev[3].record()
    packed.cpu()
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)], sum(sizes)


def measure(label, conv, tiles_d, exifs, runs, lines):
    plan = conv.converter._plan()
    want, _, _ = pillow_route(tiles_d, exifs)  # warm-up, and the bytes to hold the device route to
    got, _ = device_route(conv, tiles_d, exifs)
    assert got == want, "the two routes disagree"
    a = [pillow_route(tiles_d, exifs)[1:] for _ in range(runs)]
    b = [device_route(conv, tiles_d, exifs)[1] for _ in range(runs)]
    stages = [device_stages(plan, tiles_d) for _ in range(runs)]
    a_total, b_total = statistics.median(x + y for x, y in a) * 1e3, statistics.median(b) * 1e3
    n = tiles_d.shape[0]
    lines += [
        f"{label}: {n} tiles of {tiles_d.shape[1]} x {tiles_d.shape[2]}, {tiles_d.numel() / 1e6:.1f} MB of RGB -> {sum(map(len, want)) / 1e6:.2f} MB of JPEG files",
        f"  (a) download + Pillow save loop: {a_total:9.2f} ms   (download {statistics.median(x for x, _ in a) * 1e3:.2f} ms, "
        f"save {statistics.median(y for _, y in a) * 1e3:.2f} ms = {statistics.median(y for _, y in a) * 1e3 / n:.3f} ms per tile)",
        f"  (b) jpeg_bytes_from_images:      {b_total:9.2f} ms   ({a_total / b_total:.1f}x; {n / b_total * 1e3:.0f} tiles/s)",
        "      device stages (events): encode kernels {:.3f} ms   read of the sizes {:.3f} ms   gather {:.3f} ms   download {:.3f} ms".format(
            *[statistics.median(s[0][i] for s in stages) for i in range(4)]) + f"   ({stages[0][1] / 1e6:.2f} MB of scans)",
    ]
    return a_total, b_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.txt"))
    args = ap.parse_args()
    assert args.runs >= 5
    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False), device="cuda")
    plan = conv.converter._plan()
    lines = [f"JPEG files (quality 75, Pillow's defaults) from tiles on the device, to host bytes; device {torch.cuda.get_device_name(0)}, "
             f"Pillow {Image.__version__}, median of {args.runs} runs after warm-up; same file bytes on both routes"]
    tiles = torch.from_numpy(synthetic_tiles_u8(64)).to(plan.device)
    a64, b64 = measure("synthetic noise", conv, tiles, [None] * 64, args.runs, lines)
    seg = audio_util.PcmSegment(make_track(240.0, 48000), 48000)
    starts = audio_util.clip_start_times(240.0, 5.0, 0.2, max_duration_s=240.0)
    img, mx = conv.spectrogram_images_from_audio_clips(seg, starts, 5.0, return_device=True)
    exifs = [conv.exif_with_max_value(v) for v in mx.cpu().numpy()]
    measure("240 s track (tools/probe_encode_clips.py), with EXIF", conv, img, exifs, args.runs, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    assert b64 < a64, "the device route is not faster than the Pillow route for 64 tiles"


if __name__ == "__main__":
    main()
