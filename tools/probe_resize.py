"""
Times the tile resize (rfx_image_resize_u8) on the GPU: 64 mono tiles 512 -> 501 wide (audio-to-audio's step back from the
pipeline's output) and 501 -> 512 (its widening), BICUBIC, checked once against PIL.Image.resize.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/probe_resize.py` for the kernel's own time; it also prints HIP-event
medians per call.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "riffusion-hobby_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from riffusion.spectrogram_image_converter import SpectrogramImageConverter  # noqa: E402
from riffusion.spectrogram_params import SpectrogramParams  # noqa: E402


def main() -> None:
    conv = SpectrogramImageConverter(SpectrogramParams(), device="cuda")
    rng = np.random.default_rng(0)
    out = {}
    for src_w, dst_w in [(512, 501), (501, 512)]:
        tiles = torch.from_numpy(rng.integers(0, 256, size=(64, 512, src_w, 3), dtype=np.uint8)).cuda()
        got = conv.resize_images(tiles, (dst_w, 512), Image.BICUBIC)
        want = np.asarray(Image.fromarray(tiles[13].cpu().numpy()).resize((dst_w, 512), Image.BICUBIC))
        assert np.array_equal(got[13].cpu().numpy(), want)
        times = []
        for _ in range(50):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            conv.resize_images(tiles, (dst_w, 512), Image.BICUBIC)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        out[f"{src_w}->{dst_w}"] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
