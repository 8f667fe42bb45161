"""
PNG files from tiles: SpectrogramImageConverter.png_bytes_from_images (filtering, deflate stream and checksums on the device, only
the file bytes downloaded) against the loop of Pillow's `Image.save(f, "PNG")`, default and `compress_type=zlib.Z_RLE`, in one run
on one box, all ending in host `bytes` that reopen to the same pixels.

    python tools/probe_png.py [--runs 5] [--out profiles/png_encode.txt]

Workload: 64 tiles of 512 x 512 derived from the four mono golden seed tiles (each rolled along the time axis by multiples of 29
columns: spectrogram texture, 64 different tiles), written as RGB and, mode auto, as greyscale.  The device route is timed host to
host (tiles in host memory to files in host memory) with the host clock, its stages with events on the stream; medians of --runs
runs after one warm-up.  The Pillow loops run on the same host in the same run.  The first section needs no GPU: the size of
the emulator's file (the device's bytes: tests/test_gpu_png.py) over Pillow's Z_RLE file for every spectrogram golden tile.
"""
import argparse
import io
import os
import statistics
import sys
import time
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import png_cases as cpu  # noqa: E402

SEEDS = ("agile.png", "marim.png", "motorway.png", "vibes.png")


def golden_derived_tiles(n=64):
    seeds = [cpu._golden(name) for name in SEEDS]
    return np.stack([np.roll(seeds[i % 4], 29 * (i // 4), axis=1) for i in range(n)])


def ratio_lines():
    lines = ["file size, emulator (= device) over Pillow save(..., compress_type=zlib.Z_RLE) of the same pixels in the same mode; bound 1.02:"]
    for name in cpu.SPECTROGRAM_TILES:
        for mode in cpu.modes_of(name):
            got, ch, stats, want = cpu._case(name, mode)
            default = len(cpu.pillow_file(cpu._tile(name), ch))
            lines.append(f"  {name:58s} {mode:4s} channels {ch}: {len(got):7d} / {len(want):7d} = {len(got) / len(want):.4f}   "
                         f"(Pillow default {default:7d}: {len(got) / default:.2f} x; blocks limited to 15 bits: {int(stats[2])})")
    return lines


def pillow_loop(tiles, channels, **options):
    t0 = time.perf_counter()
    files = [cpu.pillow_file(t, channels, **options) for t in tiles]
    return files, time.perf_counter() - t0


def device_stages(plan, tiles_d, mode):
    """rfx_png_encode_u8, the read of sizes / CRCs / channels, the gather of the used bytes, their download (ms, events)"""
    import torch

    from riffusion import _hip

    N, H, W, _ = tiles_d.shape
    lib = plan.lib
    m = _hip.PNG_MODES[mode]
    cap, need = lib.rfx_png_stream_capacity(H, W, 1 if m == 1 else 3), lib.rfx_png_encode_workspace_bytes(N, H, W)
    out = torch.empty((N, cap), dtype=torch.uint8, device=plan.device)
    ws = torch.empty(need, dtype=torch.uint8, device=plan.device)
    meta = torch.empty((3, N), dtype=torch.int32, device=plan.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    _hip.check(lib.rfx_png_encode_u8(tiles_d.data_ptr(), N, H, W, m, out.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(),
                                     ws.data_ptr(), _hip.current_stream(plan.device)))
    ev[1].record()
    sizes = [int(v) for v in meta.cpu()[0]]
    ev[2].record()
    packed = torch.cat([out[n, :s] for n, s in enumerate(sizes)])
    ev[3].record()
    packed.cpu()
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)], sum(sizes)


def gpu_lines(runs):
    import torch

    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    conv = SpectrogramImageConverter(SpectrogramParams(stereo=False), device="cuda")
    plan = conv.converter._plan()
    tiles = golden_derived_tiles(64)
    lines = [f"64 golden-derived tiles of 512 x 512 ({tiles.nbytes / 1e6:.1f} MB of RGB) to PNG files in host memory; device "
             f"{torch.cuda.get_device_name(0)}, Pillow {Image.__version__}, zlib {zlib.ZLIB_RUNTIME_VERSION}; medians of {runs} runs after one warm-up"]
    for mode, ch, pil_mode in (("rgb", 3, "RGB"), ("auto", 1, "L")):
        files = conv.png_bytes_from_images(tiles, mode=mode)  # warm-up
        for t, f in zip(tiles, files):
            back = np.asarray(Image.open(io.BytesIO(f)))
            assert np.array_equal(back, t if ch == 3 else t[:, :, 0]), "the device's file does not reopen to the tile"
        host = []
        for _ in range(runs):
            t0 = time.perf_counter()
            conv.png_bytes_from_images(tiles, mode=mode)
            host.append(time.perf_counter() - t0)
        tiles_d = torch.from_numpy(tiles).to(plan.device)
        stages = [device_stages(plan, tiles_d, mode) for _ in range(runs + 1)][1:]
        default_files, default_s = pillow_loop(tiles, ch)
        rle = [pillow_loop(tiles, ch, compress_type=zlib.Z_RLE) for _ in range(max(3, runs // 2))]
        rle_files, rle_s = rle[0][0], statistics.median(s for _, s in rle)
        dev_ms = statistics.median(host) * 1e3
        lines += [
            f"mode {mode} (Pillow mode {pil_mode}):",
            f"  device route, host to host (png_bytes_from_images): {dev_ms:9.2f} ms = {dev_ms / 64:.3f} ms per tile; files {sum(map(len, files)) / 1e6:.2f} MB",
            "      stages (events): kernels of rfx_png_encode_u8 {:.3f} ms   read of sizes, CRCs, channels {:.3f} ms   gather {:.3f} ms   download {:.3f} ms".format(
                *[statistics.median(s[0][i] for s in stages) for i in range(4)]) + f"   ({stages[0][1] / 1e6:.2f} MB of streams)",
            f"  Pillow save loop, default (level 6), one run:       {default_s * 1e3:9.2f} ms = {default_s * 1e3 / 64:.3f} ms per tile; files {sum(map(len, default_files)) / 1e6:.2f} MB"
            f"   ({default_s * 1e3 / dev_ms:.1f} x the device route's time; device files {sum(map(len, files)) / sum(map(len, default_files)):.2f} x the size)",
            f"  Pillow save loop, compress_type=zlib.Z_RLE:         {rle_s * 1e3:9.2f} ms = {rle_s * 1e3 / 64:.3f} ms per tile; files {sum(map(len, rle_files)) / 1e6:.2f} MB"
            f"   ({rle_s * 1e3 / dev_ms:.1f} x the device route's time; device files {sum(map(len, files)) / sum(map(len, rle_files)):.3f} x the size)",
        ]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.txt"))
    ap.add_argument("--sizes-only", action="store_true", help="the first section alone (no GPU)")
    args = ap.parse_args()
    lines = ratio_lines()
    if not args.sizes_only:
        lines += [""] + gpu_lines(args.runs)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
