"""
Command line front-end for the spectrogram <-> audio codec.

Same sub-commands and keyword flags as the part of the reference CLI that drives this path
(`riffusion/cli.py:23-95` audio-to-image / image-to-audio / print-exif, `:134-204`
audio-to-images-batch), but the batch commands feed whole batches to the GPU
(`SpectrogramImageConverter.spectrogram_images_from_waveforms` /
`audio_from_spectrogram_images`) instead of one clip per thread-pool task, and split the file list
over the ranks when launched one process per GPU (`python -m torch.distributed.run
--nproc-per-node 8 -m riffusion.cli images-to-audio-batch ...`).  argparse replaces argh (not
installed here); without pydub only 16-bit PCM wav files are read and only wav is written.

    python -m riffusion.cli image-to-audio --image tile.png --audio out.wav
    python -m riffusion.cli audio-to-image --audio clip.wav --image tile.png
    python -m riffusion.cli print-exif --image tile.png
    python -m riffusion.cli images-to-audio-batch --image-dir tiles/ --output-dir wavs/
    python -m riffusion.cli audio-to-images-batch --audio-dir wavs/ --output-dir tiles/
    python -m riffusion.cli time-stretch --audio clip.wav --output slower.wav --bpm-from 120 --bpm-to 100
    python -m riffusion.cli pitch-shift --audio clip.wav --output higher.wav --semitones 2
"""
import argparse
import glob
import os
import sys
import typing as T

import numpy as np
from PIL import Image

from riffusion.spectrogram_image_converter import SpectrogramImageConverter
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import audio_util, image_util


def _load_segment(path: str) -> T.Any:
    pydub = audio_util._pydub()
    if pydub is not None:
        return pydub.AudioSegment.from_file(path)
    return audio_util.PcmSegment.from_wav(path)


def _params_from_exif(exif: T.Any) -> SpectrogramParams:
    try:
        return SpectrogramParams.from_exif(exif=exif)
    except (KeyError, AttributeError):
        print("WARNING: Could not find spectrogram parameters in exif data. Using defaults.")
        return SpectrogramParams()


def _png_params_and_size(data: bytes) -> T.Optional[T.Tuple[SpectrogramParams, T.Tuple[int, int]]]:
    """(params from the eXIf chunk, (width, height)) of a PNG file's bytes, from its chunks alone (image_util.png_parse); None
    where the file is not one the device reads: the caller opens it as an image."""
    info = image_util.png_parse(data)
    if not info.ok_for_device:
        return None
    exif = Image.Exif()
    if info.exif:
        exif.load(info.exif)
    return _params_from_exif(exif), (info.width, info.height)


def _check_png_reader(png_reader: str) -> None:
    if png_reader not in _CHOICES["png_reader"]:
        raise ValueError(f"--png-reader must be one of {_CHOICES['png_reader']}, got {png_reader}")


def _params_from_image(image: Image.Image) -> SpectrogramParams:
    """EXIF -> params, defaults when the image carries none (reference cli.py:77-87)."""
    try:
        return SpectrogramParams.from_exif(exif=image.getexif())
    except (KeyError, AttributeError):
        print("WARNING: Could not find spectrogram parameters in exif data. Using defaults.")
        return SpectrogramParams()


def audio_to_image(*, audio: str, image: str, step_size_ms: int = 10, num_frequencies: int = 512, min_frequency: int = 0,
                   max_frequency: int = 10000, window_duration_ms: int = 100, padded_duration_ms: int = 400,
                   power_for_image: float = 0.25, stereo: bool = False, device: str = "cuda", frame_engine: str = "auto",
                   png_writer: str = "pillow", png_mode: str = "rgb", loop: bool = False) -> None:
    """Encode one clip; --frame-engine chirp-z runs a sample rate / padded duration whose FFT length has a prime factor above 13.
    --png-writer device writes the PNG on the GPU (lossless: the same pixels and EXIF, not Pillow's bytes; the size of zlib's Z_RLE
    strategy); with it --png-mode gray or auto writes a mono tile as greyscale, 0.63 of the RGB file.
    --loop: the clip is a loop - it is encoded on the circular STFT, its end running into its start, and gives one column per hop
    (a 5.12 s clip at 44.1 kHz: 512 columns) that image-to-audio --loop decodes to the same length.  The clip must be a whole number of
    hops long, at least the padded duration: any other length is refused with the nearest legal lengths; nothing is trimmed or padded."""
    _check_png_flags(png_writer, png_mode)
    segment = _load_segment(audio)
    params = SpectrogramParams(
        sample_rate=segment.frame_rate, stereo=stereo, window_duration_ms=window_duration_ms,
        padded_duration_ms=padded_duration_ms, step_size_ms=step_size_ms, min_frequency=min_frequency,
        max_frequency=max_frequency, num_frequencies=num_frequencies, power_for_image=power_for_image,
    )
    converter = SpectrogramImageConverter(params=params, device=device, frame_engine=frame_engine)
    pil_image = converter.spectrogram_image_from_audio(segment, loop=loop)
    if png_writer == "device":
        data = converter.png_bytes_from_images(np.asarray(pil_image)[None], exif=pil_image.getexif(), mode=png_mode)[0]
        with open(image, "wb") as f:
            f.write(data)
    else:
        pil_image.save(image, exif=pil_image.getexif(), format="PNG")
    print(f"Wrote {image}")


def _check_png_flags(png_writer: str, png_mode: str) -> None:
    if png_writer not in _CHOICES["png_writer"] or png_mode not in _CHOICES["png_mode"]:
        raise ValueError(f"--png-writer must be one of {_CHOICES['png_writer']} and --png-mode one of {_CHOICES['png_mode']}")
    if png_writer == "pillow" and png_mode != "rgb":
        raise ValueError("--png-mode gray / auto needs --png-writer device: Pillow's route writes the RGB tile as it is")


# the combination rules (`_hip.check_call_rules`) in the words of image-to-audio's flags
_FLAG_WORDING = {
    "roles": {"guide_audio": "guide", "hold_ms": "hold", "hold_mask": "hold_bins"},
    "peak_and_guide": "--phase-start peaks does not go with --guide-audio: they are two starts",
    "loop_holds": "--loop does not go with --hold-head-ms / --hold-tail-ms / --hold-mask",
    "bins_need_guide": "--hold-mask needs --guide-audio: the bins are held at the guide's phase",
    "bins_and_hold": "--hold-mask does not go with --hold-head-ms / --hold-tail-ms: paint the held frames' columns black in the mask",
    "hold_needs_guide": "--hold-head-ms / --hold-tail-ms need --guide-audio: the frames are held at the guide's phase",
}


def _check_image_to_audio(*, guide_audio: str, hold_head_ms: int, hold_tail_ms: int, hold_mask: str, loop: bool, phase_start: str,
                          print_error: bool = False, **_: T.Any) -> None:
    """ValueError for flags of image-to-audio that do not go together (the function raises it, the parser reports it)"""
    from riffusion import _hip

    _hip.check_call_rules(_FLAG_WORDING, loop=loop, peak_start=phase_start == "peaks", guide_audio=guide_audio or None,
                          hold_ms=(hold_head_ms or hold_tail_ms) or None, hold_mask=hold_mask or None)
    if hold_head_ms < 0 or hold_tail_ms < 0:
        raise ValueError("--hold-head-ms / --hold-tail-ms must be >= 0")
    if print_error and not loop:
        raise ValueError("--print-error needs --loop: it prints the circular spectral convergence of a loop decode")


def image_to_audio(*, image: str, audio: str, device: str = "cuda", inverse_mel: str = "sgd", frame_engine: str = "auto",
                   guide_audio: str = "", griffin_lim_iters: int = -1, hold_head_ms: int = 0, hold_tail_ms: int = 0,
                   hold_mask: str = "", hold_keep_threshold: float = 0.5, loop: bool = False, phase_start: str = "random",
                   print_error: bool = False, png_reader: str = "pillow") -> None:
    """Decode one spectrogram image; --inverse-mel lstsq takes the closed-form InverseMelScale (torchaudio >= 2.1's) instead of the SGD,
    --frame-engine chirp-z runs parameters whose FFT length has a prime factor above 13 (refused otherwise).
    --guide-audio FILE starts Griffin-Lim from the phase of that clip (audio-to-audio: the clip the tile was made of; it must be at
    the tile's sample rate) instead of random phases, --griffin-lim-iters N runs N iterations instead of the params' 32 (a guided
    decode needs 0 to 4).  --hold-head-ms N / --hold-tail-ms N, with --guide-audio: the first / last N milliseconds of the clip are
    known audio (a continuation's left part, the ends around a re-drawn middle) - the frames whose windows lie wholly inside them keep
    the guide's phase through the iterations instead of only starting from it.  --hold-mask MASK.png, with --guide-audio: a mask image
    of the tile's size as the reference's mask_image (black is kept, white is repainted) - the kept region keeps the guide's phase
    through the iterations; a pixel is kept where 1 - L / 255 >= --hold-keep-threshold (0.5).  Not together with the two above.
    --loop: the tile is a loop - Griffin-Lim runs on the circular STFT and the clip (hop * width samples) runs from its end into its
    start without a click; the tile needs n_fft / hop columns (40 at the defaults).  Not with --hold-head-ms / --hold-tail-ms / --hold-mask.
    --phase-start peaks starts Griffin-Lim from phases built from the tile's own magnitudes (spectral peaks, their frequencies
    integrated over the hop) instead of random ones: for a tile without a guide and few --griffin-lim-iters.  Not with --guide-audio.
    --print-error, with --loop: prints the decode's circular spectral convergence, || |STFT(x)| - S || / || S || of the clip Griffin-Lim
    made against the magnitudes it was given, the STFT being the circular one of a loop encode, measured on the device.
    --png-reader device inflates and unfilters a PNG tile on the GPU (the same pixels and EXIF; only the file's bytes are uploaded);
    a file the device does not read (16-bit, interlaced, not a PNG, a damaged stream) is opened by Pillow as with the default."""
    _check_png_reader(png_reader)
    _check_image_to_audio(guide_audio=guide_audio, hold_head_ms=hold_head_ms, hold_tail_ms=hold_tail_ms, hold_mask=hold_mask, loop=loop,
                          phase_start=phase_start, print_error=print_error)
    parsed = None
    if png_reader == "device":
        with open(image, "rb") as f:
            data = f.read()
        parsed = _png_params_and_size(data)
    if parsed is not None:
        params = parsed[0]
        converter = SpectrogramImageConverter(params=params, device=device, frame_engine=frame_engine)
        pil_image = converter.images_from_png_bytes([data], return_device=True)[0][0]  # the (H, W, 3) tile on the device
    else:
        pil_image = Image.open(image)
        params = _params_from_image(pil_image)
        converter = SpectrogramImageConverter(params=params, device=device, frame_engine=frame_engine)
    segment = converter.audio_from_spectrogram_image(pil_image, apply_filters=True, inverse_mel=inverse_mel,
                                                     guide_segment=_load_segment(guide_audio) if guide_audio else None,
                                                     griffin_lim_iters=griffin_lim_iters if griffin_lim_iters >= 0 else None,
                                                     hold_frames=params.hold_frames_for(hold_head_ms / 1000.0, hold_tail_ms / 1000.0)
                                                     if hold_head_ms or hold_tail_ms else None,
                                                     hold_mask=image_util.hold_mask_from_image(Image.open(hold_mask), hold_keep_threshold)
                                                     if hold_mask else None, loop=loop, phase_start=phase_start, return_loop_error=print_error)
    if print_error:
        segment, error = segment
        print(f"Spectral convergence (circular STFT): {error:.6f}")
    segment.export(audio, format=os.path.splitext(audio)[1][1:] or "wav")
    print(f"Wrote {audio} ({segment.duration_seconds:.2f} seconds)")


def print_exif(*, image: str) -> None:
    pil_image = Image.open(image)
    exif = image_util.exif_from_image(pil_image)
    for name, value in exif.items():
        print(f"{name:<20} = {value:>15}")


def _rank_slice(items: T.Sequence[T.Any]) -> T.Sequence[T.Any]:
    """Under `torchrun` / `torch.distributed.run` (one process per GPU) every rank converts its contiguous share of
    the files and writes its own outputs: the N-GPU form of the reference's per-file thread pool (cli.py:172-204).
    No process group is needed - files are independent and nothing is gathered."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world <= 1:
        return items
    from riffusion.batch_shard import shard_range

    lo, hi = shard_range(len(items), world, rank)
    return items[lo:hi]


def _rank_device(device: str) -> str:
    """'cuda' -> this rank's GPU when launched one process per GPU."""
    if device == "cuda" and "LOCAL_RANK" in os.environ:
        return f"cuda:{int(os.environ['LOCAL_RANK'])}"
    return device


def _tile_groups(paths: T.Sequence[str], image_extension: str, png_reader: str = "pillow") -> T.Dict[T.Tuple[SpectrogramParams, T.Tuple[int, int]], T.List[str]]:
    """Image files by (params from their EXIF, (width, height)): the tiles of one GPU call share both.  A jpg's size and EXIF come
    from the bytes before its scan (image_util.jpeg_parse), without opening it as an image; a file that does not parse is opened."""
    groups: T.Dict[T.Tuple[SpectrogramParams, T.Tuple[int, int]], T.List[str]] = {}
    for path in paths:
        if image_extension == "png" and png_reader == "device":  # (the same from the chunks, without opening the file as an image)
            with open(path, "rb") as f:
                parsed = _png_params_and_size(f.read())
            if parsed is not None:
                groups.setdefault(parsed, []).append(path)
                continue
        if image_extension != "png":
            with open(path, "rb") as f:
                info = image_util.jpeg_parse(f.read())
            if info.width and info.height:
                exif = Image.Exif()
                if info.exif:
                    exif.load(info.exif)
                try:
                    params = SpectrogramParams.from_exif(exif=exif)
                except (KeyError, AttributeError):
                    print("WARNING: Could not find spectrogram parameters in exif data. Using defaults.")
                    params = SpectrogramParams()
                groups.setdefault((params, (info.width, info.height)), []).append(path)
                continue
        with Image.open(path) as im:
            groups.setdefault((_params_from_image(im), im.size), []).append(path)
    return groups


def _load_tiles(converter: SpectrogramImageConverter, chunk: T.Sequence[str], image_extension: str, png_reader: str = "pillow") -> T.Any:
    """The (N, H, W, 3) uint8 tiles of one chunk of same-size files, opened by Pillow one by one and stacked on the host.
    jpg / jpeg files could be decoded on the device instead (`converter.images_from_jpeg_bytes(files, return_device=True)`: the
    same pixels, and only the coded bytes are uploaded); they stay on this route until tools/probe_jpeg_decode.py has written
    profiles/jpeg_decode.txt and the device route is faster there on both of its sets.  `png_reader="device"` (--png-reader device):
    the png files' bytes go to `converter.images_from_png_bytes(files, return_device=True)` instead and the tiles stay on the device."""
    if image_extension == "png" and png_reader == "device":
        files = []
        for p in chunk:
            with open(p, "rb") as f:
                files.append(f.read())
        return converter.images_from_png_bytes(files, return_device=True)[0]
    tiles = []
    for p in chunk:
        with Image.open(p) as im:
            tiles.append(image_util.rgb_array_from_image(im))
    return np.stack(tiles)


def images_to_audio_batch(*, image_dir: str, output_dir: str, batch_size: int = 64, no_filters: bool = False,
                          compression: bool = False, device: str = "cuda", inverse_mel: str = "sgd", image_extension: str = "png",
                          frame_engine: str = "auto", loop: bool = False, phase_start: str = "random", griffin_lim_iters: int = -1,
                          png_reader: str = "pillow") -> None:
    """Decode every *.png (or, with --image-extension jpg / jpeg, every file of that extension) of a directory, `batch_size`
    same-width tiles per GPU call.  Each clip then gets the same
    post-processing as `image-to-audio` (audio_util.apply_filters, reference spectrogram_image_converter.py:65-91, run on the
    device) unless --no-filters is given; --compression adds the filters' dynamic range compression (apply_filters with
    compression=True, also on the device); --inverse-mel lstsq takes the closed-form InverseMelScale instead of the SGD;
    --frame-engine chirp-z decodes tiles whose parameters give an FFT length with a prime factor above 13; --loop decodes every
    tile as a loop (see image-to-audio); --phase-start peaks starts Griffin-Lim from the tiles' spectral peaks instead of random
    phases and --griffin-lim-iters N runs N iterations instead of the params' 32: the start is for decodes with few of them.
    --png-reader device decodes the png files on the GPU (inflate, unfilter, to RGB: the same pixels, only the files' bytes are
    uploaded); files the device does not read are opened by Pillow as with the default, pillow."""
    _check_png_reader(png_reader)
    if griffin_lim_iters < -1:
        raise ValueError("--griffin-lim-iters must be >= 0")
    if compression and no_filters:
        raise ValueError("--compression is a mode of the filters: it does not go with --no-filters")
    if image_extension not in ("png", "jpg", "jpeg"):
        raise ValueError(f"--image-extension must be png, jpg or jpeg, got {image_extension}")
    os.makedirs(output_dir, exist_ok=True)
    device = _rank_device(device)
    paths = _rank_slice(sorted(glob.glob(os.path.join(image_dir, "*." + image_extension))))
    for (params, _size), members in _tile_groups(paths, image_extension, png_reader).items():
        converter = SpectrogramImageConverter(params=params, device=device, frame_engine=frame_engine)
        for i in range(0, len(members), batch_size):
            chunk = members[i : i + batch_size]
            # the filters run on the device, clip by clip, before the batch leaves it (same bytes as audio_util.apply_filters)
            pcm = converter.audio_from_spectrogram_images(_load_tiles(converter, chunk, image_extension, png_reader), apply_filters=not no_filters,
                                                          compression=compression, inverse_mel=inverse_mel, loop=loop, phase_start=phase_start,
                                                          griffin_lim_iters=griffin_lim_iters if griffin_lim_iters >= 0 else None)
            for path, samples in zip(chunk, pcm):
                segment = audio_util.PcmSegment(samples, params.sample_rate)
                out = os.path.join(output_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
                segment.export(out, format="wav")
            print(f"Wrote {len(chunk)} clips to {output_dir}")


def _device_convertible(seg: T.Any, sample_rate: int) -> bool:
    """Can Plan.resample_pcm stand in for seg.set_channels(...).set_frame_rate(sample_rate)?  16-bit mono or stereo, a rate pair
    whose reduced rates stay below 2^20 (include/rfx.h), and a length the clip entry's int holds; anything else keeps the host path."""
    import math

    if seg.sample_width != 2 or seg.channels not in (1, 2):
        return False
    g = math.gcd(int(seg.frame_rate), int(sample_rate))
    if max(int(seg.frame_rate), int(sample_rate)) // g >= audio_util.RATECV_RATE_LIMIT:
        return False
    return 0 < audio_util.ratecv_frames(int(seg.frame_count()), int(seg.frame_rate), int(sample_rate)) < (1 << 31)


def audio_to_images_batch(*, audio_dir: str, output_dir: str, image_extension: str = "jpg", step_size_ms: int = 10,
                          num_frequencies: int = 512, min_frequency: int = 0, max_frequency: int = 10000,
                          power_for_image: float = 0.25, mono: bool = False, sample_rate: int = 44100, device: str = "cuda",
                          num_threads: int = 0, limit: int = -1, batch_size: int = 64, frame_engine: str = "auto",
                          png_writer: str = "pillow", png_mode: str = "rgb") -> None:
    """Process audio clips into spectrogram images in batch (reference cli.py:134-204, same flags and defaults: stereo
    tiles unless --mono, files resampled to --sample-rate, unreadable files skipped, jpg output - encoded on the device, the same
    bytes as Pillow's; png is written by Pillow on the host unless --png-writer device, which writes it on the GPU: lossless, the
    same pixels and EXIF, not Pillow's bytes; --png-mode gray / auto then writes mono tiles as greyscale).  Instead of one clip
    per thread-pool task (`num_threads` is accepted and ignored) same-length clips go to the GPU `batch_size` at a time.  A file
    whose channel count or rate differs is mixed and resampled on the device (Plan.resample_pcm), same bytes as pydub's.
    --frame-engine chirp-z runs a --sample-rate whose FFT length has a prime factor above 13."""
    import torch

    _check_png_flags(png_writer, png_mode)
    os.makedirs(output_dir, exist_ok=True)
    device = _rank_device(device)
    image_format = {"jpg": "JPEG", "jpeg": "JPEG", "png": "PNG"}[image_extension]
    paths = sorted(p for p in glob.glob(os.path.join(audio_dir, "*")) if os.path.isfile(p))
    if limit > 0:
        paths = paths[:limit]
    paths = _rank_slice(paths)
    params = SpectrogramParams(step_size_ms=step_size_ms, num_frequencies=num_frequencies, min_frequency=min_frequency,
                               max_frequency=max_frequency, power_for_image=power_for_image, stereo=not mono,
                               sample_rate=sample_rate)
    converter = SpectrogramImageConverter(params=params, device=device, frame_engine=frame_engine)
    channels = 1 if mono else 2
    # Streaming: files are decoded one at a time and grouped by sample count (a GPU call needs equal lengths); a group is
    # converted and released as soon as it holds `batch_size` clips, and when the waveforms held - in host memory, or in device
    # memory for files that were converted there: one budget for both - pass `max_pending_bytes` the LARGEST group is flushed early - a directory of long clips of many different lengths never
    # sits in RAM as a whole (the reference streams one file per thread-pool task, cli.py:172-204).
    max_pending_bytes = 2 << 30
    pending: T.Dict[int, T.List[T.Tuple[str, np.ndarray]]] = {}
    pending_bytes = 0

    def flush(n_samples: int) -> None:
        nonlocal pending_bytes
        chunk = pending.pop(n_samples)
        pending_bytes -= sum(w.nbytes for _, w in chunk)
        if all(isinstance(w, np.ndarray) for _, w in chunk):  # files that matched: one host stack, one upload
            batch = torch.from_numpy(np.stack([w for _, w in chunk]))
        else:  # a file converted on the device left its waveform there: the host ones of its group join it
            plan = converter.converter._plan()
            batch = torch.stack([w if isinstance(w, torch.Tensor) else torch.from_numpy(w).to(plan.device) for _, w in chunk])
        if image_format == "JPEG" or png_writer == "device":
            if image_format == "JPEG":  # encoded on the device: the bytes of the image.save below, and only they are downloaded
                files, _ = converter.spectrogram_images_from_waveforms(batch, as_jpeg=True)
            else:  # written on the device: the pixels and EXIF of the image.save below in a stream of its own
                files, _ = converter.spectrogram_images_from_waveforms(batch, as_png=True, png_mode=png_mode)
            for (path, _), data in zip(chunk, files):
                with open(os.path.join(output_dir, os.path.splitext(os.path.basename(path))[0] + "." + image_extension), "wb") as f:
                    f.write(data)
            print(f"Wrote {len(chunk)} images to {output_dir}")
            return
        images, max_values = converter.spectrogram_images_from_waveforms(batch)
        for (path, _), image, mx in zip(chunk, images, max_values):
            exif_data = params.to_exif()
            exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(mx)
            image.getexif().update(exif_data.items())
            out = os.path.join(output_dir, os.path.splitext(os.path.basename(path))[0] + "." + image_extension)
            image.save(out, exif=image.getexif(), format=image_format)
        print(f"Wrote {len(chunk)} images to {output_dir}")

    for path in paths:
        try:
            seg = _load_segment(path)
        except Exception:  # the reference skips files it cannot read (cli.py:176-179)
            continue
        if (seg.channels != channels or seg.frame_rate != params.sample_rate) and _device_convertible(seg, params.sample_rate):
            # set_channels, then set_frame_rate (reference cli.py:181-187) on the device, byte for byte: the int16 samples go up
            # once and come back as the (channels, samples) float32 waveform, which stays there until its group is converted
            plan = converter.converter._plan()
            data = np.asarray(seg.get_array_of_samples(), dtype=np.int16).reshape(-1, seg.channels)
            pcm = plan.resample_pcm(torch.from_numpy(np.ascontiguousarray(data)).to(plan.device), int(seg.frame_rate), params.sample_rate,
                                    out_channels=channels)
            wave = plan.clips_to_waveform(pcm, [0], int(pcm.shape[0]), channels)
        else:
            if seg.channels != channels:  # (more than two channels: pydub's own reduction, on the host)
                seg = seg.set_channels(channels)
            if seg.frame_rate != params.sample_rate:
                seg = seg.set_frame_rate(params.sample_rate)
            wave = np.array([c.get_array_of_samples() for c in seg.split_to_mono()]).astype(np.float32)
        del seg
        group = pending.setdefault(wave.shape[1], [])
        group.append((path, wave))
        pending_bytes += wave.nbytes
        if len(group) >= batch_size:
            flush(wave.shape[1])
        while pending_bytes > max_pending_bytes and pending:
            flush(max(pending, key=lambda n: sum(w.nbytes for _, w in pending[n])))
    for n_samples in sorted(pending):
        flush(n_samples)


def _stretch_rate(*, rate: float, bpm_from: float, bpm_to: float, **_: T.Any) -> float:
    """the rate of time-stretch from its flags: --rate R, or --bpm-from A --bpm-to B (rate B / A); ValueError for flags that do not
    go together (the function raises it, the parser reports it)"""
    by_bpm = bool(bpm_from) or bool(bpm_to)
    if bool(rate) == by_bpm:
        raise ValueError("time-stretch takes either --rate R or --bpm-from A --bpm-to B")
    if by_bpm:
        if not (bpm_from > 0 and bpm_to > 0) or bpm_from == float("inf") or bpm_to == float("inf"):
            raise ValueError("--bpm-from and --bpm-to must both be given, finite and positive")
        return bpm_to / bpm_from
    if not rate > 0 or rate == float("inf"):
        raise ValueError("--rate must be finite and positive")
    return rate


def time_stretch(*, audio: str, output: str, rate: float = 0.0, bpm_from: float = 0.0, bpm_to: float = 0.0, device: str = "cuda",
                 frame_engine: str = "auto") -> None:
    """Play a clip faster or slower at the same pitch: the phase vocoder between the STFT and its inverse, on the device.
    --rate R: R times as fast (1.25: a fifth shorter; 0.8: a quarter longer), or --bpm-from A --bpm-to B: a clip at A beats per
    minute comes out at B (rate B / A).  The clip's channels are rows of one call; the result is peak-normalised into 16-bit PCM as a
    decode's is.  The analysis runs at the clip's sample rate with the default window, hop and padding.  One rate for the whole clip;
    a loop does not stay a loop (the accumulated phase does not close at the loop point)."""
    import torch

    from riffusion.spectrogram_converter import SpectrogramConverter

    r = _stretch_rate(rate=rate, bpm_from=bpm_from, bpm_to=bpm_to)
    segment = _load_segment(audio)
    waveform = np.array([c.get_array_of_samples() for c in segment.split_to_mono()]).astype(np.float32)
    params = SpectrogramParams(sample_rate=int(segment.frame_rate), stereo=waveform.shape[0] == 2)
    converter = SpectrogramConverter(params=params, device=device, frame_engine=frame_engine)
    stretched = converter.time_stretch(torch.from_numpy(waveform), r)
    pcm, _ = converter._plan().pcm16(stretched, channels=stretched.shape[0], normalize=True)
    out = audio_util.segment_from_pcm16(pcm[0].cpu().numpy(), params.sample_rate)
    out.export(output, format=os.path.splitext(output)[1][1:] or "wav")
    print(f"Wrote {output} ({out.duration_seconds:.2f} seconds, rate {r:.4f})")


def _semitones(*, semitones: T.Union[str, float], **_: T.Any) -> float:
    """the shift of pitch-shift from its flag (a required flag arrives as text): ValueError for one that is no finite number (the
    function raises it, the parser reports it)"""
    try:
        n = float(semitones)
    except (TypeError, ValueError):
        raise ValueError(f"--semitones must be a number, got {semitones!r}") from None
    if n != n or n in (float("inf"), float("-inf")):
        raise ValueError("--semitones must be finite")
    return n


def pitch_shift(*, audio: str, output: str, semitones: T.Union[str, float], device: str = "cuda", frame_engine: str = "auto") -> None:
    """Move a clip to another key at the same tempo and duration: the time stretch, then the band-limited resampler back to the
    clip's length, on the device.  --semitones N: N semitones up (negative: down; 12 is an octave; fractions are allowed).  The
    clip's channels are rows of one call; the result is peak-normalised into 16-bit PCM as a decode's is.  The analysis runs at
    the clip's sample rate with the default window, hop and padding.  One shift for the whole clip; a loop does not stay a loop."""
    import torch

    from riffusion.spectrogram_converter import SpectrogramConverter

    n = _semitones(semitones=semitones)
    segment = _load_segment(audio)
    waveform = np.array([c.get_array_of_samples() for c in segment.split_to_mono()]).astype(np.float32)
    params = SpectrogramParams(sample_rate=int(segment.frame_rate), stereo=waveform.shape[0] == 2)
    converter = SpectrogramConverter(params=params, device=device, frame_engine=frame_engine)
    shifted = converter.pitch_shift(torch.from_numpy(waveform), n)
    pcm, _ = converter._plan().pcm16(shifted, channels=shifted.shape[0], normalize=True)
    out = audio_util.segment_from_pcm16(pcm[0].cpu().numpy(), params.sample_rate)
    out.export(output, format=os.path.splitext(output)[1][1:] or "wav")
    print(f"Wrote {output} ({out.duration_seconds:.2f} seconds, {n:+g} semitones)")


_COMMANDS: T.Dict[str, T.Callable[..., None]] = {
    "audio-to-image": audio_to_image,
    "image-to-audio": image_to_audio,
    "print-exif": print_exif,
    "images-to-audio-batch": images_to_audio_batch,
    "audio-to-images-batch": audio_to_images_batch,
    "time-stretch": time_stretch,
    "pitch-shift": pitch_shift,
}


_CHOICES = {"inverse_mel": ("sgd", "lstsq"), "frame_engine": ("auto", "chirp-z"), "phase_start": ("random", "peaks"),
            "png_writer": ("pillow", "device"), "png_mode": ("rgb", "gray", "auto"), "png_reader": ("pillow", "device")}  # arguments that take one of a few words


def build_parser() -> argparse.ArgumentParser:
    import inspect

    parser = argparse.ArgumentParser(prog="riffusion.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest="command", required=True)
    for name, fn in _COMMANDS.items():
        sp = sub.add_parser(name, help=(fn.__doc__ or "").strip().split("\n")[0])
        for arg, spec in inspect.signature(fn).parameters.items():
            flag = "--" + arg.replace("_", "-")
            if spec.default is inspect.Parameter.empty:
                sp.add_argument(flag, required=True)
            elif isinstance(spec.default, bool):
                sp.add_argument(flag, action="store_true", default=spec.default)
            else:
                sp.add_argument(flag, type=type(spec.default), default=spec.default, choices=_CHOICES.get(arg))
    return parser


def main(argv: T.Optional[T.Sequence[str]] = None) -> None:
    parser = build_parser()
    args = vars(parser.parse_args(argv))
    command = args.pop("command")
    if command == "image-to-audio":
        try:
            _check_image_to_audio(**args)
        except ValueError as e:
            parser.error(str(e))
        if args["hold_mask"] and not 0.0 <= args["hold_keep_threshold"] <= 1.0:
            parser.error("--hold-keep-threshold must be in [0, 1]")
    if command in ("audio-to-image", "audio-to-images-batch"):
        try:
            _check_png_flags(args["png_writer"], args["png_mode"])
        except ValueError as e:
            parser.error(str(e))
    if command == "time-stretch":
        try:
            _stretch_rate(**args)
        except ValueError as e:
            parser.error(str(e))
    if command == "pitch-shift":
        try:
            _semitones(**args)
        except ValueError as e:
            parser.error(str(e))
    if command == "images-to-audio-batch" and args["griffin_lim_iters"] < -1:
        parser.error("--griffin-lim-iters must be >= 0")
    if command == "audio-to-image" and args["loop"]:
        from riffusion.spectrogram_converter import LoopLengthError

        try:  # (a clip that is no whole loop is a usage error: the message names the nearest lengths that are)
            return audio_to_image(**args)
        except LoopLengthError as e:
            parser.error(str(e))
    _COMMANDS[command](**args)


if __name__ == "__main__":
    main(sys.argv[1:])
