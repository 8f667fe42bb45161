"""
Spectrogram images <-> audio segments.

Drop-in for the reference's `riffusion/spectrogram_image_converter.py:10-91` (same constructor,
attributes and the two per-clip methods) plus batch entry points that keep many tiles in flight on
the GPU: `audio_from_spectrogram_images` takes uint8 tiles in and hands int16 PCM out with one H2D
and one D2H copy per batch, takes the diffusion pipeline's output tensors directly
(`riffusion_pipeline.py:427-434`), and shards a batch of clips over the ranks of a
`torch.distributed` process group (one process per GPU; clips are independent, so the only
collective is the final all_gather of the int16 PCM).
"""
import functools
import io
import typing as T

import numpy as np
import torch
from PIL import Image

from riffusion import _hip
from riffusion._decode import ClipExtras
from riffusion.spectrogram_converter import CALL_WORDING, SpectrogramConverter, hold_mask_rows, hold_rows
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import audio_util, image_util


# ... and of the batch entry points, whose guides are `guide_waveforms`
BATCH_WORDING = {**CALL_WORDING, "hold_needs_guide": "hold_frames needs guide_waveforms: the frames are held at the guides' phase",
                 "bins_need_guide": "hold_mask needs guide_waveforms: the bins are held at the guides' phase"}
_RANGE_MSG = "float images must be the pipeline's [0, 1] output (riffusion_pipeline.py:427-431); pass 0..255 pixel values as uint8"


class _FileFormat(T.NamedTuple):
    """What `_images_from_files` needs to know of a file format."""
    parse: T.Callable  # a file -> its info: `ok_for_device`, `exif` and what the two below read
    key: T.Callable  # an info -> what the files of one device call share
    decode: T.Callable  # (plan, the call's files, their infos, their key) -> (rgb, status)


def _jpeg_group_decode(plan: T.Any, files: T.List[bytes], infos: T.List[T.Any], key: T.Tuple[int, int]) -> T.Tuple[torch.Tensor, np.ndarray]:
    return plan.jpeg_decode([f[info.scan[0]:info.scan[1]] for f, info in zip(files, infos)], *key,
                            np.stack([info.qtables for info in infos]), np.stack([info.huffman for info in infos]))


def _png_group_decode(plan: T.Any, files: T.List[bytes], infos: T.List[T.Any], key: T.Tuple[int, int, int]) -> T.Tuple[torch.Tensor, np.ndarray]:
    streams = [b"".join(f[a:b] for a, b in info.idat) for f, info in zip(files, infos)]
    paletted = key[2] == 3
    return plan.png_decode(streams, *key, np.stack([info.palette for info in infos]) if paletted else None,
                           np.array([info.palette_entries for info in infos], dtype=np.int32) if paletted else None)


_JPEG_FILES = _FileFormat(image_util.jpeg_parse, lambda info: (info.height, info.width), _jpeg_group_decode)
_PNG_FILES = _FileFormat(image_util.png_parse, lambda info: (info.height, info.width, info.color_type), _png_group_decode)


class SpectrogramImageConverter:
    def __init__(self, params: SpectrogramParams, device: str = "cuda", *, frame_engine: str = "auto"):
        """`frame_engine="chirp-z"`: as SpectrogramConverter's - parameter sets "auto" refuses for their FFT length run on the chirp-z engine."""
        self.p = params
        self.device = device
        self.converter = SpectrogramConverter(params=params, device=device, frame_engine=frame_engine)

    # ---- reference API: one clip per call -------------------------------------------------------------
    def spectrogram_image_from_audio(self, segment: T.Any, loop: bool = False) -> Image.Image:
        """Audio segment -> spectrogram image carrying the params (and MAX_VALUE) as EXIF.  `loop`: the segment is one period of a
        loop, exactly hop * T samples (any other length raises ValueError with the nearest legal lengths: nothing is trimmed or
        padded), and is encoded on the circular STFT (`spectrogram_images_from_waveforms`): a tile of T columns that closes."""
        assert int(segment.frame_rate) == self.p.sample_rate, "Sample rate mismatch"

        if self.p.stereo:
            if segment.channels == 1:
                print("WARNING: Mono audio but stereo=True, cloning channel")
                segment = segment.set_channels(2)
            elif segment.channels > 2:
                print("WARNING: Multi channel audio, reducing to stereo")
                segment = segment.set_channels(2)
        else:
            if segment.channels > 1:
                print("WARNING: Stereo audio but stereo=False, setting to mono")
                segment = segment.set_channels(1)

        waveform = np.array([c.get_array_of_samples() for c in segment.split_to_mono()]).astype(np.float32)
        images, max_values = self.spectrogram_images_from_waveforms(torch.from_numpy(waveform)[None], loop=loop)
        image = images[0]
        exif_data = self.p.to_exif()
        exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(max_values[0])
        image.getexif().update(exif_data.items())
        return image

    def audio_from_spectrogram_image(
        self,
        image: Image.Image,
        apply_filters: bool = True,
        max_value: float = 30e6,
        *,
        inverse_mel: str = "sgd",
        guide_segment: T.Any = None,
        griffin_lim_iters: T.Optional[int] = None,
        hold_frames: T.Optional[T.Tuple[int, int]] = None,
        hold_mask: T.Any = None,
        loop: bool = False,
        phase_start: str = "random",
        return_loop_error: bool = False,
    ) -> T.Any:
        """Spectrogram image -> audio segment (the EXIF MAX_VALUE is not read back, like the reference).  The filters
        (audio_util.apply_filters, compression=False) run on the device: same bytes.  `inverse_mel`: "sgd" (default) or
        "lstsq", as in `audio_from_spectrogram_images`.  `guide_segment`: a PcmSegment or pydub segment at the params' sample
        rate (ValueError otherwise) whose phase starts Griffin-Lim - the clip the tile was made of, in audio-to-audio; mono
        guides both channels of a stereo tile, more channels than the tile's are mixed down.  `griffin_lim_iters`: iterations for
        this call in place of the params' (a guided decode needs few).  `hold_frames`: with a guide, the `(head, tail)` frames at
        the clip's two ends that keep the guide's phase through the iterations (`hold_frames_for` turns seconds of known audio
        into the pair).  `hold_mask`: with a guide, a mask image of the tile's size (black is kept, as the reference's `mask_image`)
        or an (n_mels, W) boolean array: the kept region keeps the guide's phase through the iterations.  `loop`: the tile is
        one period of a loop: hop * W samples whose end runs into their start (not with `hold_frames` / `hold_mask`).
        `phase_start`: "random" (default) or "peaks", Griffin-Lim's start built from the tile's magnitudes (not with a guide).  All as
        in `audio_from_spectrogram_images`.  `return_loop_error=True` (only with `loop=True`, ValueError otherwise) returns
        (segment, error): the clip's circular spectral convergence as a float, `audio_from_spectrogram_images`' `return_loop_error`;
        same audio."""
        _hip.check_call_rules(CALL_WORDING, "peak_start", "hold_needs_guide", "bins_need_guide", peak_start=_hip.check_phase_start(phase_start),
                              guide_segment=guide_segment, hold_frames=hold_frames, hold_mask=hold_mask)
        guides = None
        if guide_segment is not None:
            if int(guide_segment.frame_rate) != self.p.sample_rate:
                raise ValueError(f"guide_segment is at {guide_segment.frame_rate} Hz, the params say {self.p.sample_rate} Hz: resample it first")
            C = 2 if self.p.stereo else 1
            if guide_segment.channels > C:
                guide_segment = guide_segment.set_channels(C)
            guides = np.array([c.get_array_of_samples() for c in guide_segment.split_to_mono()]).astype(np.float32)[None]
        # (a PIL image, or its (H, W, 3) uint8 tile as an array or a device tensor: what `images_from_png_bytes` returns)
        tile = np.asarray(image_util.rgb_array_from_image(image)) if isinstance(image, Image.Image) else image
        pcm = self.audio_from_spectrogram_images(
            tile[None], max_value=max_value, apply_filters=apply_filters,
            inverse_mel=inverse_mel, guide_waveforms=guides, griffin_lim_iters=griffin_lim_iters, hold_frames=hold_frames,
            hold_mask=hold_mask, loop=loop, phase_start=phase_start, return_loop_error=return_loop_error,
        )
        if return_loop_error:
            return audio_util.segment_from_pcm16(pcm[0][0], self.p.sample_rate), float(pcm[1][0])
        return audio_util.segment_from_pcm16(pcm[0], self.p.sample_rate)

    def hold_frames_for(self, head_s: float = 0.0, tail_s: float = 0.0) -> T.Tuple[int, int]:
        """`SpectrogramParams.hold_frames_for` of this converter's params: the `hold_frames` pair for `head_s` / `tail_s` seconds
        of known audio at a clip's two ends."""
        return self.p.hold_frames_for(head_s, tail_s)

    # ---- batch entry points ------------------------------------------------------------------------------
    def _filter_pcm(self, plan: T.Any, pcm: torch.Tensor, compression: bool = False) -> torch.Tensor:
        """audio_util.apply_filters on each clip of an (n, L, C) int16 device batch, in place: on the device where its arithmetic
        equals audioop's (L * C < 2^23), otherwise on the host, clip by clip."""
        _, L, C = pcm.shape
        if L * C < audio_util.FILTER_EXACT_SAMPLES:
            return plan.apply_filters(pcm, out=pcm, compression=compression)
        host = pcm.cpu().numpy()
        for i in range(host.shape[0]):
            seg = audio_util.apply_filters(audio_util.PcmSegment(host[i], self.p.sample_rate), compression=compression)
            host[i] = seg.get_array_of_samples().reshape(L, C)
        pcm.copy_(torch.from_numpy(host))
        return pcm

    def audio_from_spectrogram_image_sequence(
        self,
        images: T.Any,
        crossfade_s: float = 0.2,
        apply_filters: bool = True,
        max_value: float = 30e6,
        seed: T.Optional[int] = None,
        tiles_per_call: int = 64,
        return_device: bool = False,
        compression: bool = False,
        size: T.Optional[T.Tuple[int, int]] = None,
        return_error: bool = False,
        *,
        inverse_mel: str = "sgd",
        guide_waveforms: T.Any = None,
        griffin_lim_iters: T.Optional[int] = None,
        hold_mask: T.Any = None,
        loop: bool = False,
        phase_start: str = "random",
    ) -> T.Any:
        """
        A sequence of tiles -> ONE audio segment: every tile decoded (`audio_from_spectrogram_images`), filtered
        (`apply_filters`, on the device) and the clips joined with `crossfade_s` of crossfade - the reference's audio-to-audio
        (crossfade 0.2 s) and interpolation (crossfade 0) consumers, streamlit/tasks/audio_to_audio.py:323-324 and
        interpolation.py:177-181.  Byte for byte
        `audio_util.stitch_segments([audio_util.apply_filters(clip, compression) for clip in
        audio_from_spectrogram_images(images, seed=seed)], crossfade_s)`; the stitch runs on the device too (rfx_pcm16_stitch, from audio_util.stitch_plan's pieces).
        `images`: what `audio_from_spectrogram_images` takes, or a sequence of PIL images of one size.  Raises append's ValueError
        when the crossfade is longer than a clip; one tile gives that clip.  Returns a pydub segment when pydub is importable,
        else a PcmSegment; with `return_device=True` the (frames, C) int16 tensor on the GPU.  All clips are stitched in this
        process: there is no `group`.
        `size=(width, height)`: every tile is first resized as `Image.resize(size, Image.BICUBIC)` does, on the device (see
        `audio_from_spectrogram_images`); the stitch is planned for the clips of that width.  Tiles of different sizes in a list
        (without `size`) are decoded one by one, each with the random starts of its index in the sequence, and stitched on the
        host.
        `return_error=True` returns (segment, errors): the per-clip spectral convergence of `audio_from_spectrogram_images`
        ((n,) float64; a device tensor with `return_device=True`); the segment's bytes do not change.  Not for tiles of
        different sizes without `size`.
        `inverse_mel`: "sgd" (default) or "lstsq", as in `audio_from_spectrogram_images`.
        `guide_waveforms`, `griffin_lim_iters`, `hold_mask`: the guides of a phase-guided decode, its iterations and the kept
        region of a partial regeneration, as in `audio_from_spectrogram_images`; not for tiles of different sizes without `size`.
        `phase_start`: "random" (default) or "peaks", as in `audio_from_spectrogram_images`; not for tiles of different sizes
        without `size`.
        """
        _hip.check_inverse_mel(inverse_mel)
        peaks = _hip.check_phase_start(phase_start)
        rules = functools.partial(_hip.check_call_rules, BATCH_WORDING, peak_start=peaks, guide_waveforms=guide_waveforms, hold_mask=hold_mask)
        rules("peak_start")
        if loop:  # (`loop` is here to be refused: a sequence is stitched with crossfades, its clips do not repeat)
            raise ValueError("loop does not go with a stitched sequence: decode loops with audio_from_spectrogram_images(loop=True)")
        rules("bins_need_guide")
        if isinstance(images, (list, tuple)):
            arrays = [np.asarray(image_util.rgb_array_from_image(im)) if isinstance(im, Image.Image) else np.asarray(im)
                      for im in images]
            if len({a.shape for a in arrays}) > 1:
                if size is None:
                    if return_error:
                        raise ValueError("return_error needs tiles of one size (or `size`): clips decoded one by one carry no error figure")
                    if guide_waveforms is not None or griffin_lim_iters is not None:
                        raise ValueError("guide_waveforms / griffin_lim_iters need tiles of one size (or `size`)")
                    if peaks:
                        raise ValueError('phase_start="peaks" needs tiles of one size (or `size`)')
                    return self._image_sequence_mixed(arrays, crossfade_s, apply_filters, max_value, seed, return_device, compression,
                                                      inverse_mel=inverse_mel)
                images, size = torch.cat([self.resize_images(a[None], size) for a in arrays]), None
            else:
                images = np.stack(arrays)
        n = int(images.shape[0])
        if n < 1:
            raise ValueError("audio_from_spectrogram_image_sequence needs at least one image")
        plan = self.converter._plan()
        L = plan.lib.rfx_griffinlim_output_samples(plan.handle, int(size[0]) if size is not None else int(images.shape[2]))
        C = 2 if self.p.stereo else 1
        try:  # the lengths alone decide whether the stitch can be planned: before any GPU work
            audio_util.stitch_plan(n, L, self.p.sample_rate, crossfade_s)
            on_device = True
        except audio_util.StitchNotPlannable:  # a crossfade that reaches into the previous one: pydub's own loop, on the host
            on_device = False
        pcm = self.audio_from_spectrogram_images(images, max_value=max_value, seed=seed, tiles_per_call=tiles_per_call,
                                                 return_device=True, apply_filters=apply_filters, compression=compression, size=size,
                                                 return_error=return_error, inverse_mel=inverse_mel, guide_waveforms=guide_waveforms,
                                                 griffin_lim_iters=griffin_lim_iters, hold_mask=hold_mask, phase_start=phase_start)
        errors = None
        if return_error:
            pcm, errors = pcm
            if not return_device:
                errors = errors.cpu().numpy()
        if n == 1:
            joined = pcm[0]
        elif on_device:
            joined = plan.stitch(pcm, self.p.sample_rate, crossfade_s)
        else:
            segs = [audio_util.PcmSegment(clip, self.p.sample_rate) for clip in pcm.cpu().numpy()]
            joined = torch.from_numpy(audio_util.stitch_segments(segs, crossfade_s).get_array_of_samples().reshape(-1, C).copy())
            joined = joined.to(plan.device)
        if not return_device:
            joined = audio_util.segment_from_pcm16(joined.cpu().numpy(), self.p.sample_rate)
        return (joined, errors) if return_error else joined

    def _image_sequence_mixed(self, arrays: T.List[np.ndarray], crossfade_s: float, apply_filters: bool, max_value: float,
                              seed: T.Optional[int], return_device: bool, compression: bool, inverse_mel: str = "sgd") -> T.Any:
        """audio_from_spectrogram_image_sequence of tiles whose widths differ: clip i is decoded alone with the random starts of
        row i (clip_base), as it would be in one batch, filtered on the device, and the clips are stitched on the host."""
        self._check_compression(compression, apply_filters)
        conv = self.converter
        plan = conv._plan()
        lstsq = _hip.check_inverse_mel(inverse_mel)
        if lstsq:
            plan.require_lstsq()
        lut, max_value = self._decode_lut(plan, max_value)
        base_seed = conv._seed(seed)
        segs = []
        for i, a in enumerate(arrays):
            tile = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))[None].to(plan.device)
            pcm = plan.audio_from_image(tile, self.p.stereo, lut, self.p.num_griffin_lim_iters, 0.99, seed=base_seed, normalize=True,
                                        clip_base=i, magnitude_hint=max_value, lstsq=lstsq)[0]
            if apply_filters:
                pcm = self._filter_pcm(plan, pcm, compression)
            segs.append(audio_util.PcmSegment(pcm[0].cpu().numpy(), self.p.sample_rate))
        C = 2 if self.p.stereo else 1
        joined = audio_util.stitch_segments(segs, crossfade_s).get_array_of_samples().reshape(-1, C)
        if return_device:
            return torch.from_numpy(joined.copy()).to(plan.device)
        return audio_util.segment_from_pcm16(joined, self.p.sample_rate)

    def spectrogram_images_from_waveforms(self, waveforms: torch.Tensor, return_device: bool = False, *,
                                          as_jpeg: bool = False, as_png: bool = False, png_mode: str = "rgb",
                                          loop: bool = False) -> T.Tuple[T.Any, T.Any]:
        """(N, C, samples) float waveforms at int16 scale -> N RGB images and their float32 MAX_VALUEs.  With
        `return_device=True` the (N, n_mels, T, 3) uint8 tensor and the (N,) float32 maxima as they are on the GPU (no copy, no
        synchronisation): the encode side of audio-to-audio's device chain.  With `as_jpeg=True` the images come back as N JPEG
        files (`bytes`), encoded on the device (`jpeg_bytes_from_images`), each with the params and its MAX_VALUE as EXIF: the
        bytes of `image.save(f, exif=image.getexif(), format="JPEG")` on `spectrogram_image_from_audio`'s image.  With
        `as_png=True` they come back as N PNG files, lossless, written on the device (`png_bytes_from_images` with
        `mode=png_mode`) with the same EXIF: any reader gets `spectrogram_image_from_audio`'s pixels back.
        `loop=True`: every waveform is one period of a loop - exactly hop * T samples, hop * T >= n_fft; any other length raises
        ValueError with the nearest legal lengths in samples and milliseconds, nothing is trimmed or padded - and the tiles are made
        on the circular STFT (rfx_image_from_waveform_loop): T columns, column 0 follows column T - 1, and
        `audio_from_spectrogram_images(loop=True)` decodes clips of the same hop * T samples.  Goes with every output form."""
        self._check_file_outputs(as_jpeg, as_png, return_device)
        conv = self.converter
        plan = conv._plan()
        N, C, L = waveforms.shape
        if C != (2 if self.p.stereo else 1):
            raise ValueError(f"expected {2 if self.p.stereo else 1} channel(s), got {C}")
        if loop:
            conv.check_loop_samples(int(L))
        power = float(self.p.power_for_image)
        thr = plan.device_constant(("encode_thresholds", power), lambda: image_util.encode_thresholds(power))
        # one call (rfx_image_from_waveform): the mel amplitudes go from the forward kernel to the encoder without the (N*C, M, T) tensor
        img, mx = plan.image_from_waveform(waveforms.reshape(N * C, L).to(conv.device, torch.float32), self.p.stereo, thr, loop=loop)
        return self._deliver_tiles(img, mx, return_device, as_jpeg, as_png, png_mode)

    def _deliver_tiles(self, tiles: T.Any, maxima: torch.Tensor, return_device: bool, as_jpeg: bool, as_png: bool, png_mode: str) -> T.Tuple[T.Any, T.Any]:
        """Tiles on the device - one (N, n_mels, T, 3) batch, or a list of N tiles whose widths differ - and their (N,) maxima in
        the form the caller asked for: as they are, as JPEG or PNG files with the params and MAX_VALUE as EXIF, or as PIL images."""
        if return_device:
            return tiles, maxima
        mx_np = maxima.cpu().numpy()
        if as_jpeg or as_png:
            encode = self.jpeg_bytes_from_images if as_jpeg else functools.partial(self.png_bytes_from_images, mode=png_mode)
            exifs = [self.exif_with_max_value(v) for v in mx_np]
            if isinstance(tiles, list):
                return [encode(t[None], exif=e)[0] for t, e in zip(tiles, exifs)], mx_np
            return (encode(tiles, exif=exifs) if len(exifs) else []), mx_np
        host = [t.cpu().numpy() for t in tiles] if isinstance(tiles, list) else tiles.cpu().numpy()
        return [Image.fromarray(a, mode="RGB") for a in host], mx_np

    # ---- JPEG files from tiles on the device: Pillow's Image.save(f, "JPEG"), byte for byte (rfx_jpeg_encode_u8) ----------------
    def exif_with_max_value(self, max_value: float) -> Image.Exif:
        """The EXIF `spectrogram_image_from_audio` attaches to a tile: the params and the tile's MAX_VALUE."""
        exif_data = self.p.to_exif()
        exif_data[SpectrogramParams.ExifTags.MAX_VALUE.value] = float(max_value)
        exif = Image.Exif()
        exif.update(exif_data.items())
        return exif

    def jpeg_bytes_from_images(self, images: T.Any, exif: T.Any = None, quality: int = 75, *, subsampling: T.Any = None,
                               optimize: T.Any = None, progressive: T.Any = None, tiles_per_call: int = 64) -> T.List[bytes]:
        """
        (N, H, W, 3) uint8 tiles (a tensor on any device, or an array) -> N JPEG files as `bytes`, byte-equal to
        `Image.fromarray(t).save(f, "JPEG", quality=quality, exif=e)`: baseline, 4:2:0, libjpeg's tables for `quality` (1 .. 100)
        and the standard Huffman tables.  The colour conversion, the DCT, the quantisation and the entropy coding run on the
        device (rfx_jpeg_encode_u8) and only the coded bytes are downloaded; the header is built on the host
        (`image_util.jpeg_header`).  `exif`: None, one `Image.Exif` (or its bytes) for every tile, or a sequence of N.
        Pillow's `subsampling`, `optimize` and `progressive` are not implemented: giving one raises ValueError.  The tiles are
        encoded `tiles_per_call` at a time: the scans' worst-case buffer is about 2.5 MB per 512 x 512 tile.
        """
        imgs, exifs = self._tiles_to_encode(
            images, exif, image_util.jpeg_exif_bytes, tiles_per_call, "jpeg_bytes_from_images writes Pillow's default baseline 4:2:0 files only",
            subsampling=subsampling, optimize=optimize, progressive=progressive)
        quality = int(quality)
        if not 1 <= quality <= 100:
            raise ValueError(f"quality must be in 1 .. 100, got {quality}")
        plan = self.converter._plan()
        N, H, W, _ = imgs.shape
        head, tail = image_util.jpeg_header_parts(W, H, quality, _hip.jpeg_quant_tables(quality))
        files: T.List[bytes] = []
        for lo in range(0, N, tiles_per_call):
            chunk = imgs[lo:lo + tiles_per_call]
            for e, scan in zip(exifs[lo:lo + tiles_per_call], plan.jpeg_scans(chunk.to(plan.device), quality)):
                files.append(b"".join((head, image_util._jpeg_segment(0xE1, e) if e else b"", tail, scan)))
        return files

    @staticmethod
    def _tiles_to_encode(images: T.Any, exif: T.Any, exif_bytes: T.Callable[[T.Any], bytes], tiles_per_call: int, writes: str,
                         **unimplemented: T.Any) -> T.Tuple[torch.Tensor, T.List[bytes]]:
        """The front of `jpeg_bytes_from_images` / `png_bytes_from_images`: refuses the keywords of Pillow's the writer does not
        implement and a `tiles_per_call` below 1 -> the checked (N, H, W, 3) uint8 tensor and `exif` as N `exif_bytes` strings."""
        for name, value in unimplemented.items():
            if value is not None:
                raise ValueError(f"{writes}: `{name}` is not implemented")
        if tiles_per_call < 1:
            raise ValueError(f"tiles_per_call must be >= 1, got {tiles_per_call}")
        if not isinstance(images, torch.Tensor):
            images = np.ascontiguousarray(images)
            images = images if images.flags.writeable else images.copy()  # (torch takes no read-only arrays, such as a PIL image's)
        imgs = _hip.check_tiles(torch.as_tensor(images))
        N = imgs.shape[0]
        if exif is None or isinstance(exif, (Image.Exif, bytes, bytearray)):
            return imgs, [exif_bytes(exif)] * N
        exifs = [exif_bytes(e) for e in exif]
        if len(exifs) != N:
            raise ValueError(f"{N} images need {N} EXIF entries (or one for all), got {len(exifs)}")
        return imgs, exifs

    # ---- PNG files from tiles on the device: lossless, the IDAT payload written there (rfx_png_encode_u8) --------------------------
    @staticmethod
    def _check_file_outputs(as_jpeg: bool, as_png: bool, return_device: bool) -> None:
        if as_jpeg and as_png:
            raise ValueError("as_jpeg and as_png both name the files to return: give one")
        if (as_jpeg or as_png) and return_device:
            raise ValueError(f"{'as_jpeg' if as_jpeg else 'as_png'} returns files on the host: it does not go with return_device=True")

    def png_bytes_from_images(self, images: T.Any, exif: T.Any = None, *, mode: str = "rgb", tiles_per_call: int = 64,
                              optimize: T.Any = None, compress_level: T.Any = None, compress_type: T.Any = None,
                              bits: T.Any = None) -> T.List[bytes]:
        """
        (N, H, W, 3) uint8 tiles (a tensor on any device, or an array) -> N PNG files as `bytes`, lossless: `Image.open` gives
        the tile's pixels and the EXIF back.  Filtering, the deflate stream (run-length + Huffman, the size of Pillow's
        `compress_type=zlib.Z_RLE`; csrc/rfx_png_core.h), its Adler-32 and the IDAT chunk's CRC-32 are computed on the device
        (rfx_png_encode_u8) and only the file's bytes are downloaded; the chunks around the payload are built on the host
        (`image_util.png_file`) as Pillow lays them out.  The IDAT bytes are NOT zlib's: the file is not byte-equal to Pillow's.
        `mode`: "rgb" writes colour type 2; "gray" colour type 0 (channel 0) and raises ValueError naming the first tile whose
        channels differ; "auto" writes each tile grey where R = G = B at every pixel and RGB otherwise, decided on the device.
        `exif`: None, one `Image.Exif` (or its bytes) for every tile, or a sequence of N.  Pillow's `optimize`, `compress_level`,
        `compress_type` and `bits` are not implemented: giving one raises ValueError.  The tiles are encoded `tiles_per_call` at
        a time: the streams' worst-case buffer and the scratch space are about 4 MB per 512 x 512 tile.
        """
        imgs, exifs = self._tiles_to_encode(
            images, exif, image_util.png_exif_bytes, tiles_per_call, "png_bytes_from_images writes its own run-length + Huffman stream only",
            optimize=optimize, compress_level=compress_level, compress_type=compress_type, bits=bits)
        if mode not in _hip.PNG_MODES:
            raise ValueError(f"mode must be one of {sorted(_hip.PNG_MODES)}, got {mode!r}")
        plan = self.converter._plan()
        N, H, W, _ = imgs.shape
        files: T.List[bytes] = []
        for lo in range(0, N, tiles_per_call):
            streams, crcs, channels = plan.png_streams(imgs[lo:lo + tiles_per_call].to(plan.device), mode)
            for k, (stream, crc, ch) in enumerate(zip(streams, crcs, channels)):
                if ch == 0:
                    raise ValueError(f"mode='gray': tile {lo + k} is not grey (its channels differ); use mode='auto' or 'rgb'")
                files.append(image_util.png_file(W, H, int(ch), stream, int(crc), exifs[lo + k]))
        return files

    # ---- tiles from JPEG files, decoded on the device: np.asarray(Image.open(f).convert("RGB")), byte for byte (rfx_jpeg_decode_u8) --
    def images_from_jpeg_bytes(self, files: T.Sequence[bytes], return_device: bool = False, tiles_per_call: int = 64) -> T.Tuple[T.Any, T.List[Image.Exif]]:
        """
        N image files as `bytes` -> (their (H, W, 3) uint8 tiles, their EXIF as `Image.Exif`).  A baseline 4:2:0 JPEG
        (`image_util.jpeg_parse(...).ok_for_device`: what Pillow's default `save` and `jpeg_bytes_from_images` write, `optimize=True`
        included) is decoded on the device, `tiles_per_call` files of one size at a time, to the pixels Pillow gives; only the coded
        bytes are uploaded.  Every other file - progressive, greyscale, other subsamplings, restart markers, not a JPEG - and every
        file whose scan the device reports as damaged is opened by Pillow on the host (`image_util.rgb_array_from_image`), with
        Pillow's own exceptions for files it cannot read.  The tiles come back as one (N, H, W, 3) batch when all files have one
        size, else as a list of N; numpy arrays, or tensors on the device with `return_device=True`.
        """
        return self._images_from_files(files, return_device, tiles_per_call, _JPEG_FILES)

    def images_from_png_bytes(self, files: T.Sequence[bytes], return_device: bool = False, tiles_per_call: int = 64) -> T.Tuple[T.Any, T.List[Image.Exif]]:
        """
        N image files as `bytes` -> (their (H, W, 3) uint8 tiles, their EXIF as `Image.Exif`): `images_from_jpeg_bytes` for PNG.
        An 8-bit PNG of colour type 0, 2, 3 or 6 that is not interlaced (`image_util.png_parse(...).ok_for_device`: what Pillow's
        `save` and `png_bytes_from_images` write) is inflated, unfiltered and converted on the device, `tiles_per_call` files of one
        size and colour type at a time, to the pixels Pillow's `convert("RGB")` gives; only the IDAT bytes are uploaded.  Every other
        file - 16-bit, interlaced, grey with alpha, APNG, a CRC mismatch, not a PNG - and every file whose stream the device reports
        a status for is opened by Pillow on the host (`image_util.rgb_array_from_image`), with Pillow's own exceptions for files it
        cannot read.  The tiles come back as one (N, H, W, 3) batch when all files have one size, else as a list of N; numpy
        arrays, or tensors on the device with `return_device=True`.
        """
        return self._images_from_files(files, return_device, tiles_per_call, _PNG_FILES)

    def _images_from_files(self, files: T.Sequence[bytes], return_device: bool, tiles_per_call: int, fmt: _FileFormat) -> T.Tuple[T.Any, T.List[Image.Exif]]:
        """`images_from_jpeg_bytes` / `images_from_png_bytes`: the files `fmt.parse` finds `ok_for_device` are decoded there,
        `tiles_per_call` files of one `fmt.key` at a time; a file is the device's when its status is 0 and Pillow's otherwise."""
        if tiles_per_call < 1:
            raise ValueError(f"tiles_per_call must be >= 1, got {tiles_per_call}")
        files = [bytes(f) for f in files]
        plan = self.converter._plan()
        infos = [fmt.parse(f) for f in files]
        tiles: T.List[T.Any] = [None] * len(files)
        exifs: T.List[T.Any] = [None] * len(files)
        groups: T.Dict[T.Any, T.List[int]] = {}
        for i, info in enumerate(infos):
            if info.ok_for_device:
                groups.setdefault(fmt.key(info), []).append(i)
        whole = None  # the one device batch that is the whole result, if there is one
        for key, members in groups.items():
            for lo in range(0, len(members), tiles_per_call):
                idx = members[lo:lo + tiles_per_call]
                rgb, status = fmt.decode(plan, [files[i] for i in idx], [infos[i] for i in idx], key)
                if len(idx) == len(files) and not status.any():
                    whole = rgb
                batch = rgb if return_device else rgb.cpu().numpy()
                for j, i in enumerate(idx):
                    if status[j] == 0:
                        tiles[i] = batch[j]
                        exifs[i] = Image.Exif()
                        if infos[i].exif:
                            exifs[i].load(infos[i].exif)
        for i, data in enumerate(files):
            if tiles[i] is None:  # the host route
                with Image.open(io.BytesIO(data)) as im:
                    arr = image_util.rgb_array_from_image(im)
                    exifs[i] = im.getexif()
                tiles[i] = torch.from_numpy(arr).to(plan.device) if return_device else arr
        if whole is not None:
            return (whole if return_device else whole.cpu().numpy()), exifs
        if len(files) and len({tuple(t.shape) for t in tiles}) == 1:
            return (torch.stack(tiles) if return_device else np.stack(tiles)), exifs
        return tiles, exifs

    def spectrogram_images_from_audio_clips(self, segment: T.Any, clip_start_times: T.Sequence[float], clip_duration_s: float,
                                            return_device: bool = False, *, as_jpeg: bool = False, as_png: bool = False,
                                            png_mode: str = "rgb", loop: bool = False) -> T.Tuple[T.Any, T.Any]:
        """
        One int16 track -> the spectrogram images of its clips: `[spectrogram_image_from_audio(c) for c in
        slice_audio_into_clips(segment.set_frame_rate(params.sample_rate), clip_start_times, clip_duration_s)]`, same image
        bytes and MAX_VALUEs, with the integer DSP on the device.  The track is uploaded once as int16; when its rate differs
        from the params' it is resampled there (Plan.resample_pcm: audioop.ratecv, byte for byte); `audio_util.clip_frame_ranges`
        resolves the reference's millisecond slicing to frame offsets, and one call gathers the clips - overlaps included - mixes
        them to the params' channel count and converts them (Plan.image_from_pcm_clips).  A clip that nothing on the device
        describes - the last clip when it takes the reference's silence branch, a slice cut short by the track's end - is built
        by `slice_audio_into_clips` on the host, append's ValueError for less than 100 ms of missing audio included, and
        converted in a call of its own: it has its own length and hence its own tile width.
        Returns what `spectrogram_images_from_waveforms` returns: the N images and their float32 MAX_VALUEs in the order of
        `clip_start_times`; with `return_device=True` the (N, n_mels, T, 3) uint8 tensor and the (N,) maxima on the GPU - or,
        when a host-built clip has another width, a list of N (n_mels, T_i, 3) tensors and the (N,) maxima.  With `as_jpeg=True`
        the N images come back as JPEG files (`bytes`) encoded on the device, each with the params and its MAX_VALUE as EXIF, as
        from `spectrogram_images_from_waveforms`; with `as_png=True` as PNG files written on the device (`png_mode`: the `mode`
        of `png_bytes_from_images`).
        `loop=True`: every clip is one period of a loop and is encoded on the circular STFT (rfx_image_from_pcm16_clips_loop).
        The clips' length in frames at the params' rate - what the reference's millisecond slicing makes of `clip_duration_s` -
        must be exactly hop * T, hop * T >= n_fft: any other length raises ValueError with the nearest legal lengths in samples and
        milliseconds, and so does a clip the track does not hold in full (nothing is trimmed or padded with silence).
        """
        self._check_file_outputs(as_jpeg, as_png, return_device)
        conv = self.converter
        plan = conv._plan()
        if segment.sample_width != 2 or segment.channels not in (1, 2):
            raise ValueError("spectrogram_images_from_audio_clips takes 16-bit mono or stereo audio")
        n = len(clip_start_times)
        C = 2 if self.p.stereo else 1
        data = np.asarray(segment.get_array_of_samples(), dtype=np.int16).reshape(-1, segment.channels)
        pcm = torch.from_numpy(np.ascontiguousarray(data)).to(plan.device)
        if int(segment.frame_rate) != self.p.sample_rate:
            pcm = plan.resample_pcm(pcm, int(segment.frame_rate), self.p.sample_rate)
        r = audio_util.clip_frame_ranges(int(pcm.shape[0]), self.p.sample_rate, clip_start_times, clip_duration_s)
        if loop and n:
            # a loop clip is the `frames` frames from the frame its start time falls on, all of them inside the track: the reference's
            # silence branch - which a last clip of 5.12 s takes for one millisecond of float rounding - does not exist here
            conv.check_loop_samples(int(r.frames))
            starts = np.array([int(int(t * 1000) * (self.p.sample_rate / 1000.0)) for t in clip_start_times], dtype=np.int64)
            for i, a in enumerate(starts):
                if a < 0 or a + r.frames > int(pcm.shape[0]):
                    raise ValueError(f"loop=True: clip {i} (frames {int(a)} .. {int(a) + int(r.frames)}) reaches past the track's end "
                                     f"({int(pcm.shape[0])} frames); a loop clip is not padded with silence")
            r = r._replace(index=np.arange(n, dtype=np.int64), starts=starts, host_index=np.array([], dtype=np.int64), last_short=False)
        power = float(self.p.power_for_image)
        thr = plan.device_constant(("encode_thresholds", power), lambda: image_util.encode_thresholds(power))
        tiles: T.List[T.Any] = [None] * n
        maxima = torch.empty(n, dtype=torch.float32, device=plan.device)
        if len(r.index):
            img, mx = plan.image_from_pcm_clips(pcm, r.starts, r.frames, self.p.stereo, thr, loop=loop)
            index = torch.from_numpy(r.index).to(plan.device)
            maxima[index] = mx
            for j, i in enumerate(r.index):
                tiles[i] = img[j]
        if len(r.host_index):
            # the track as the host path would see it after set_frame_rate (the device's bytes are audioop's)
            track = segment if int(segment.frame_rate) == self.p.sample_rate else audio_util.PcmSegment(pcm.cpu().numpy(), self.p.sample_rate)
            clips = audio_util.slice_audio_into_clips(track, clip_start_times, clip_duration_s)
            for i in r.host_index:
                clip = clips[i].set_channels(C)
                wave = np.array([c.get_array_of_samples() for c in clip.split_to_mono()]).astype(np.float32)
                img, mx = self.spectrogram_images_from_waveforms(torch.from_numpy(wave)[None], return_device=True)
                tiles[i], maxima[i] = img[0], mx[0]
        if n == 0:
            tiles = torch.empty((0, plan.n_mels, 0, 3), dtype=torch.uint8, device=plan.device)
        elif len(r.index) == n:
            tiles = img  # every clip came from the one device call: its batch as it is
        elif len({int(t.shape[1]) for t in tiles}) == 1:
            tiles = torch.stack(tiles)
        return self._deliver_tiles(tiles, maxima, return_device, as_jpeg, as_png, png_mode)

    # ---- resizing tiles on the device: PIL.Image.resize, byte for byte (rfx_image_resize_u8) --------------------------------
    def resize_images(self, images: T.Any, size: T.Tuple[int, int], resample: int = Image.BICUBIC) -> torch.Tensor:
        """
        (N, H, W, 3) uint8 tiles (a tensor on any device, or an array) -> (N, height, width, 3) uint8 tensor on the converter's
        device, byte-equal to `[Image.fromarray(t).resize(size, resample) for t in images]`; `size` is PIL's (width, height) and
        `resample` one of Image.BICUBIC, Image.LANCZOS, Image.BILINEAR (Pillow's 8-bit convolution resample, libImaging/Resample.c).
        Every tile is resized on its own: a tile's bytes do not depend on the batch it travels in.
        """
        plan = self.converter._plan()
        imgs = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        width, height = int(size[0]), int(size[1])
        return plan.resize_images(imgs.to(plan.device), height, width, int(resample))

    def scale_images_to_32_stride(self, images: T.Any) -> torch.Tensor:
        """The reference's `scale_image_to_32_stride` (streamlit/tasks/audio_to_audio.py:419-425) on every tile: BICUBIC to the
        next multiple of 32 on both axes (501 x 512 -> 512 x 512 for a 5 s clip at 44.1 kHz); tiles already there are copied."""
        _, H, W, _ = images.shape
        return self.resize_images(images, (int(np.ceil(W / 32) * 32), int(np.ceil(H / 32) * 32)), Image.BICUBIC)

    def pipeline_input_from_images(self, images: T.Any) -> torch.Tensor:
        """
        The diffusion pipeline's `preprocess_image` (riffusion_pipeline.py:439-452) on the device: a LANCZOS resize of every
        tile to the floor multiple of 32 (a copy for tiles already there), `/ 255` in float32, `2x - 1`, NCHW.  (N, H, W, 3)
        uint8 -> (N, 3, H', W') float32, bitwise the reference's values: a pixel's value depends on its byte alone, so it is
        read from a 256-entry table built with the reference's own numpy / torch operations.
        """
        _, H, W, _ = images.shape
        x = self.resize_images(images, (W - W % 32, H - H % 32), Image.LANCZOS)
        lut = self.converter._plan().device_constant(("pipeline_input_lut",), image_util.pipeline_input_lut)
        return lut[x.long()].permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def quantize_pipeline_images(images: torch.Tensor) -> torch.Tensor:
        """
        The diffusion pipeline's hand-off (`riffusion_pipeline.py:427-434`): the VAE output is moved to
        [0, 1] and NHWC float32 (`(image / 2 + 0.5).clamp(0, 1)`, `.permute(0, 2, 3, 1)`), then
        `numpy_to_pil` quantises it with `(images * 255).round().astype("uint8")`.  This does that
        quantisation on whatever device the tensor lives on (round-half-to-even like numpy, float32
        like the reference), so the decoder can take the tensor without the `.cpu()` -> PIL -> numpy
        -> `.to(device)` round trip.  (N, H, W, 3) float in [0, 1] -> (N, H, W, 3) uint8.
        """
        if images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError("expected (N, H, W, 3) images, channels last, as riffusion_pipeline.py:431 produces them")
        return (images.to(torch.float32) * 255).round().to(torch.uint8)

    def audio_from_spectrogram_images(
        self,
        images_u8: T.Union[np.ndarray, torch.Tensor],
        max_value: float = 30e6,
        seed: T.Optional[int] = None,
        return_waveform: bool = False,
        group: T.Any = None,
        tiles_per_call: int = 64,
        gather: T.Optional[str] = None,
        return_device: bool = False,
        validate: T.Optional[bool] = None,
        return_range_flag: bool = False,
        apply_filters: bool = False,
        compression: bool = False,
        size: T.Optional[T.Tuple[int, int]] = None,
        return_error: bool = False,
        *,
        inverse_mel: str = "sgd",
        guide_waveforms: T.Any = None,
        griffin_lim_iters: T.Optional[int] = None,
        hold_frames: T.Any = None,
        hold_mask: T.Any = None,
        loop: bool = False,
        phase_start: str = "random",
        return_loop_error: bool = False,
    ) -> T.Any:
        """
        (N, H, W, 3) RGB tiles -> (n, samples, C) int16 PCM (or, with `return_waveform`, the (n, C, samples)
        float waveforms); a numpy array on the host, or with `return_device=True` a tensor that never left the GPU.

        `images_u8` is a uint8 array / tensor on any device, or the diffusion pipeline's float [0, 1]
        NHWC tensor (quantised here like `numpy_to_pil`, see `quantize_pipeline_images`; a float input
        with values outside [0, 1] - or NaN - is refused: pass pixel values as uint8).  `validate` says when
        that range check runs: None (default) at once for a host tensor, and for a device tensor as a flag
        computed on the device and read where the call synchronises anyway (the copy of the result to the
        host) - no host sync on the one-tile-per-request path; True: at once, with a host sync; False: never
        (`return_device=True` with a device input never synchronises and so cannot raise: there None turns a failed check
        into an all-zero result - silence, not garbage audio - and attaches the device flag as `result.range_ok`; with
        `return_range_flag=True` the call returns `(result, range_ok)` instead, the flag as a value of its own: an attribute
        does not survive slicing, `.to()` or a gather).
        Host tiles are uploaded chunk by chunk through pinned memory on a side stream (`batch_shard.ChunkSource`).

        `group`: a `torch.distributed` process group (or True for the default group).  Every rank
        passes the SAME full batch; rank r converts clips `shard_range(N, world, r)` on its own GPU
        (a clip's channels never leave their rank: they share the SGD loss mean and the peak
        normalisation), `tiles_per_call` clips at a time.  `gather` says which clips a rank RETURNS
        (`batch_shard.result_rows`):
            "none"  (default, also `None`) the own shard only, no collective at all: each rank writes / serves its own
                    clips, as the reference's consumers do (server.py:159-183, cli.py:172-204) - the mode that scales;
            "rank0" the whole batch on the group's rank 0 (one RCCL gather), the own shard elsewhere;
            "all"   the whole batch on every rank - one RCCL all_gather_into_tensor of the int16 PCM (round 2-3 default:
                    every rank receives and copies all N clips, so it does not scale; ask for it explicitly).
        Host results are staged through pinned memory; without a collective each chunk's device-to-host
        copy runs on a side stream while the next chunk computes (`batch_shard.ChunkSink`).
        With a `seed`, a clip's audio is a function of (the clip, the seed, the clip's index in `images_u8`) alone - the same
        bytes whatever `tiles_per_call` is and however many ranks share the batch (round 6: the random starts are keyed by
        the clip's global row, and nothing in the kernels' arithmetic depends on the batch a clip travels in).  Without one the
        seed is drawn from torch's global generator, like the reference's random starts (in a group: pass a seed, or seed
        torch identically on every rank).
        `apply_filters=True` gives every clip the reference's post-processing (audio_util.apply_filters, compression=False:
        gain to -12 dBFS, peak normalisation with 0.1 dB headroom) on the device, byte for byte, before the clip leaves the GPU
        (rfx_pcm16_apply_filters; clips of 2^23 samples or more - over three minutes - are filtered on the host instead).  It
        works per clip, so a clip's bytes still do not depend on the chunking or the sharding; not with `return_waveform`.
        `compression=True` (only with `apply_filters=True`) is apply_filters(compression=True): normalize, gain to -10 dBFS and
        pydub's compress_dynamic_range first, on the device as well (rfx_pcm16_apply_filters_compressed, which synchronises the
        stream once per chunk of `tiles_per_call` clips).
        `size=(width, height)` first resizes every tile as `Image.resize(size, Image.BICUBIC)` does, on the device (after the
        quantisation of a float input) - audio-to-audio's step back from the pipeline's 512-wide output to the clip's own width
        (streamlit/tasks/audio_to_audio.py:287).  The clip length then follows that width; the resize is per tile, so a clip's
        bytes still do not depend on the chunking or the sharding.
        `return_error=True` returns (result, errors): `errors` is the (n,) float64 spectral convergence of every clip,
        sqrt(sum over the clip's channels of || |STFT(x)| - S ||^2 / sum over them of || S ||^2), of the float waveform x
        Griffin-Lim produced against the linear magnitudes S InverseMelScale handed it - before peak normalisation and int16
        truncation; a numpy array, or with `return_device=True` a tensor on the GPU (then `(result, errors)` comes before
        `return_range_flag`'s flag: `(result, errors, range_ok)`).  The chunk then goes through the separate stages (decode,
        InverseMelScale, Griffin-Lim, `Plan.spectral_error`, PCM) instead of the one fused call: `result` is byte for byte the
        result without the flag, and a clip's error does not depend on `tiles_per_call` (rfx_spectral_error is batch-invariant).
        A silent target gives 0.0 (silent audio) or inf.  Not with `group`.
        `inverse_mel="lstsq"` takes torchaudio >= 2.1's InverseMelScale - relu of the minimum-norm least-squares solution,
        computed in closed form on the device (rfx_inverse_mel_lstsq) - in place of the SGD ("sgd", the default: the bytes
        of every release so far).  It needs no iterations and no random start, the bins outside the bank are zeros, and a clip's
        audio still depends on (the clip, the seed, its index) alone: Griffin-Lim's phases come from the seed as before.  Works
        with every other option.  A bank it does not serve (`Plan.lstsq_ok`) raises ValueError with the library's reason before
        any GPU work; any other value raises ValueError.
        `guide_waveforms`: (N, C, Lg) float32 or int16 waveforms, an array or a tensor on any device, in any units - tile i's
        Griffin-Lim starts from the phase of guide i's STFT instead of random phases (rfx_guided_call_options).  In an
        audio-to-audio workflow the guides are the source clips the tiles were made of: their phase is nearly right already, and
        a guided decode at 0 to 4 iterations reconstructs better than the random start at 32 (README: phase-guided decode).  C is
        the tiles' channel count, or 1: a mono guide serves both channels of a stereo tile.  A guide is cut, or zero-padded at
        its end, to the clip length; a silent guide row gives a silent row, a padded tail starts silent and is filled by the
        iterations.  Guides are chunked and sharded with their tiles and go with every other option; Griffin-Lim then has no
        randomness (with "lstsq" the whole decode has none).
        `griffin_lim_iters`: Griffin-Lim iterations of this call in place of `params.num_griffin_lim_iters`, guided or not.
        `hold_frames`: with guides, a `(head, tail)` pair for all clips or an (N, 2) integer array or tensor: the first `head` and
        the last `tail` frames of clip i (both channel rows) keep guide i's phase through every iteration instead of only starting
        from it (rfx_held_call_options), so known audio at a clip's ends - a continuation's left part, the kept ends of a partial
        regeneration - does not move, and costs no iteration work.  `hold_frames_for(head_s, tail_s)` gives the pair for seconds of
        known audio; values are clamped to the tiles' frame count.  Without guides: ValueError.  Chunks and shards slice it like
        the guides.
        `hold_mask`: with guides and without `hold_frames`, the kept region of a partial regeneration (rfx_masked_call_options):
        a PIL mask image as the reference's `mask_image` - black is kept, white is repainted (`image_util.hold_mask_from_image`,
        no resizing: the caller resizes it to the tiles' size) - or one (n_mels, W) boolean array for all clips, or an
        (N, n_mels, W) array or tensor on any device, in spectrogram orientation (band 0 first), nonzero = held.  The linear bins
        every one of whose mel bands is held at a frame keep guide i's phase there through every iteration, on both channel rows
        of a stereo clip; the magnitudes stay the tiles'.  With `size=`, W is `size[0]`.  A mask removes no iteration work.
        Without guides, with `hold_frames`, or in another shape: ValueError before any GPU work.  Chunks and shards slice it like
        the guides.
        `loop=True`: every tile is one period of a loop (rfx_loop_call_options) - what the reference's web app plays on repeat.
        Griffin-Lim runs on the circular STFT (frames modulo hop * W samples, circular overlap-add), a clip has hop * W samples
        and its last sample runs into its first: no click at the loop point.  W (or `size[0]`) must reach n_fft / hop (40 columns
        at the defaults).  Guides, `inverse_mel`, `apply_filters`, `tiles_per_call`, `group` and `size` work as without it; not
        with `hold_frames`, `hold_mask` or `return_error` (the error entry analyses with the reflect-padded STFT): ValueError.
        `return_loop_error=True` (only with `loop=True`: ValueError otherwise) is `return_error` for loop decodes: it returns
        (result, errors) with every clip's CIRCULAR spectral convergence - the clip re-analysed by the circular STFT a loop encode
        runs (rfx_spectral_error_loop) against the magnitudes Griffin-Lim was handed.  The chunk goes through the separate stages as
        under `return_error`; `result` is byte for byte the result without the flag.  Not with `group`.
        `phase_start`: "random" (default: the reference's U[0,1) phases from `seed`) or "peaks": Griffin-Lim starts every row from
        phases built from its magnitudes alone - the spectral peaks of every frame, their interpolated frequencies integrated
        over the hop (rfx_start_call_options) - so that a text-to-audio decode, which has no guide, needs fewer iterations:
        combine it with a small `griffin_lim_iters` (README: what it saves and what it costs).  Griffin-Lim then has no
        randomness (the SGD InverseMelScale still draws its start from `seed`); any `tiles_per_call` and sharding give the same
        bytes.  Not with `guide_waveforms`, `hold_frames` or `hold_mask`; any other string: ValueError before any GPU work.
        """
        from riffusion import batch_shard

        lstsq = _hip.check_inverse_mel(inverse_mel)
        peaks = _hip.check_phase_start(phase_start)
        rules = functools.partial(_hip.check_call_rules, BATCH_WORDING, loop=loop, peak_start=peaks, guide_waveforms=guide_waveforms,
                                  hold_frames=hold_frames, hold_mask=hold_mask)
        rules("peak_start", "loop_holds")
        if loop and return_error:
            raise ValueError("loop does not go with return_error=True: the spectral error is measured with the reflect-padded STFT")
        if return_loop_error and not loop:
            raise ValueError("return_loop_error=True is the circular spectral error of a loop decode: it needs loop=True")
        want_error = return_error or return_loop_error

        if tiles_per_call < 1:
            raise ValueError(f"tiles_per_call must be >= 1, got {tiles_per_call}")
        self._check_compression(compression, apply_filters)
        if return_waveform and apply_filters:
            raise ValueError("apply_filters works on int16 PCM: it does not go with return_waveform=True")
        if return_range_flag and not return_device:
            raise ValueError("return_range_flag goes with return_device=True (a host result raises on a failed range check instead)")
        if want_error and group is not None:
            raise ValueError(f"{'return_error' if return_error else 'return_loop_error'} does not go with `group`: the errors of a sharded batch are not gathered")
        if gather is None:
            gather = batch_shard.default_gather(group)
        if gather not in batch_shard.GATHER_MODES:
            raise ValueError(f"gather must be one of {batch_shard.GATHER_MODES}, got {gather!r}")

        # the arguments go together: what every chunk shares
        conv = self.converter
        plan = conv._plan()
        if lstsq:
            plan.require_lstsq()
        imgs, range_ok = self._quantised(images_u8, validate)
        n_total = imgs.shape[0]
        clips = self._clip_extras(plan, rules, n_total, int(size[0]) if size is not None else int(imgs.shape[2]), guide_waveforms, hold_frames,
                                  hold_mask, griffin_lim_iters, loop=loop, peak_start=peaks, inverse_mel=inverse_mel)
        if size is not None:
            size = (int(size[0]), int(size[1]))
        width = size[0] if size is not None else int(imgs.shape[2])
        if loop:
            _hip.check_loop_frames(plan.hop_length, plan.n_fft, width)
        L = plan.output_samples(width, loop)
        base_seed = conv._seed(seed)
        lut, max_value = self._decode_lut(plan, max_value)
        pg = None if group is None else batch_shard._resolve_group(group)
        world = 1 if group is None else torch.distributed.get_world_size(pg)
        # a shard that takes part in a collective stays on the device until the collective has run
        collective = world > 1 and gather != "none"

        # this rank's shard, chunk by chunk
        error_sums: T.Optional[T.List[torch.Tensor]] = [] if want_error else None  # per chunk the (clips, 2) sums, a clip's channels added
        convert = functools.partial(self._convert_shard, plan, imgs, clips, size=size, samples=L, lut=lut, max_value=max_value, seed=base_seed,
                                    tiles_per_call=tiles_per_call, to_host=not (collective or return_device), return_waveform=return_waveform,
                                    apply_filters=apply_filters, compression=compression, error_sums=error_sums)
        result = batch_shard.sharded_map(convert, n_total, group, gather)
        errors = None
        if want_error:
            sums = torch.cat(error_sums) if error_sums else torch.zeros((0, 2), dtype=torch.float64, device=plan.device)
            errors = conv.convergence_from_sums(sums[:, 0], sums[:, 1])
        return self._deliver(plan, result, errors, range_ok, return_device, return_range_flag)

    @staticmethod
    def _check_compression(compression: bool, apply_filters: bool) -> None:
        if compression and not apply_filters:
            raise ValueError("compression=True is a mode of the filters: it needs apply_filters=True")

    def _decode_lut(self, plan: T.Any, max_value: float) -> T.Tuple[torch.Tensor, float]:
        """(the image path's lookup table for `max_value` on the plan's device, `max_value` as a float)"""
        power, max_value = float(self.p.power_for_image), float(max_value)
        if not (max_value > 0.0 and max_value < float("inf")):
            raise ValueError(f"max_value must be a positive finite number, got {max_value}")
        return plan.device_constant(("decode_lut", power, max_value), lambda: image_util.decode_lut(power, max_value)), max_value

    def _quantised(self, images_u8: T.Any, validate: T.Optional[bool]) -> T.Tuple[torch.Tensor, T.Optional[torch.Tensor]]:
        """`audio_from_spectrogram_images`' tiles as (the uint8 tensor, the device flag of a deferred range check or None)"""
        imgs = torch.as_tensor(np.ascontiguousarray(images_u8) if isinstance(images_u8, np.ndarray) else images_u8)
        range_ok = None
        if imgs.is_floating_point():
            if imgs.numel() and validate is not False:
                ok = ((imgs >= 0) & (imgs <= 1.0 + 1e-6)).all()  # NaN compares false
                if validate or not imgs.is_cuda:
                    if not bool(ok):
                        raise ValueError(_RANGE_MSG)
                else:
                    range_ok = ok
            imgs = self.quantize_pipeline_images(imgs)
        return imgs, range_ok

    def _clip_extras(self, plan: T.Any, rules: T.Callable[..., None], n: int, width: int, guide_waveforms: T.Any, hold_frames: T.Any,
                     hold_mask: T.Any, griffin_lim_iters: T.Optional[int], **flags: T.Any) -> ClipExtras:
        """`audio_from_spectrogram_images`' per-clip arguments for n tiles of `width` columns as the value its chunks are lowered
        from.  `rules`: the entry's combination rules, checked between the arguments' own checks in the entry's order."""
        C = 2 if self.p.stereo else 1
        n_iter = self.p.num_griffin_lim_iters if griffin_lim_iters is None else int(griffin_lim_iters)
        if n_iter < 0:
            raise ValueError(f"griffin_lim_iters must be >= 0, got {griffin_lim_iters}")
        guides = None
        if guide_waveforms is not None:
            guides = torch.as_tensor(np.ascontiguousarray(guide_waveforms) if isinstance(guide_waveforms, np.ndarray) else guide_waveforms)
            if guides.dim() != 3 or guides.shape[0] != n or guides.shape[1] not in (1, C) or guides.shape[2] < 1:
                raise ValueError(f"guide_waveforms must be ({n}, {C} or 1, samples), got {tuple(guides.shape)}")
            if guides.dtype not in (torch.float32, torch.int16):
                raise ValueError(f"guide_waveforms must be float32 or int16, got {guides.dtype}")
        rules("hold_needs_guide")
        holds = hold_rows(hold_frames, n, width) if hold_frames is not None else None
        rules("bins_need_guide", "bins_and_hold")
        bands = None
        if hold_mask is not None:
            if isinstance(hold_mask, Image.Image):
                hold_mask = image_util.hold_mask_from_image(hold_mask)
            bands = hold_mask_rows(hold_mask, n, plan.n_mels, width)
        return ClipExtras(guides=guides, holds=holds, bands=bands, n_iter=n_iter, **flags)

    def _convert_shard(self, plan: T.Any, imgs: torch.Tensor, clips: ClipExtras, lo: int, hi: int, *, size: T.Optional[T.Tuple[int, int]],
                       samples: int, lut: torch.Tensor, max_value: float, seed: int, tiles_per_call: int, to_host: bool, return_waveform: bool,
                       apply_filters: bool, compression: bool, error_sums: T.Optional[T.List[torch.Tensor]]) -> torch.Tensor:
        """Tiles [lo, hi) of `audio_from_spectrogram_images`, `tiles_per_call` at a time: the (hi - lo) clips of `samples` samples as
        the entry delivers them.  One fused call per chunk (rfx_audio_from_image_u8_ex), or the stages one by one - same bytes -
        where the caller wants what lies between them: the float waveform, or (`error_sums`, a list to append every chunk's
        (clips, 2) sums to) both ends of Griffin-Lim."""
        from riffusion import batch_shard

        conv, stereo = self.converter, self.p.stereo
        C = 2 if stereo else 1
        staged = return_waveform or error_sums is not None
        row_shape, dtype = ((C, samples), torch.float32) if return_waveform else ((samples, C), torch.int16)
        sink = batch_shard.ChunkSink(hi - lo, row_shape, dtype, plan.device, to_host=to_host)
        bounds = [(a, min(hi, a + tiles_per_call)) for a in range(lo, hi, tiles_per_call)]  # bounded working set: |S| alone is 19 MB per tile-channel
        source = batch_shard.ChunkSource(imgs, bounds, plan.device)
        # (the scratch space - 1.7 GB for 64 mono tiles - comes from the plan's arena: the same buffer chunk after chunk and call after call)
        for i, (a, b) in enumerate(bounds):
            tiles = source.get(i)
            if size is not None:
                tiles = plan.resize_images(tiles, size[1], size[0], Image.BICUBIC)
            dst = None if return_waveform else sink.rows(a - lo, b - lo)  # device sink: the PCM kernel writes the batch rows in place
            if staged:
                mel = plan.image_decode(tiles, stereo, lut)
                wave = conv._waveform_from_mel(plan, mel, clips, tiles=(a, b, C), seed=seed, channels_per_clip=C, row_base=a * C,
                                               magnitude_hint=max_value, return_slots=error_sums is not None)
                if error_sums is not None:
                    wave, lin_slots = wave
                    error_sums.append(plan.spectral_error(wave, lin_slots, (b - a) * C, int(mel.shape[-1]), loop=clips.loop).reshape(b - a, C, 2).sum(1))
                out = wave.reshape(b - a, C, -1) if return_waveform else plan.pcm16(wave, C, normalize=True, out=dst)[0]
            else:
                out = plan.audio_from_image(tiles, stereo, lut, clips.n_iter, 0.99, seed=seed, normalize=True, out=dst, clip_base=a,
                                            magnitude_hint=max_value, extras=clips.rows(plan, (a, b, C), bins_first=True))[0]
            if apply_filters:  # (never with `return_waveform`)
                out = self._filter_pcm(plan, out, compression)
            # this chunk's kernels are queued: the host stages and uploads the next chunk underneath them
            source.prefetch(i + 1)
            sink.put(a - lo, b - lo, out)
        return sink.finish()  # a rank with an empty shard still joins the collective with 0 rows

    @staticmethod
    def _deliver(plan: T.Any, result: torch.Tensor, errors: T.Optional[torch.Tensor], range_ok: T.Optional[torch.Tensor], return_device: bool,
                 return_range_flag: bool) -> T.Any:
        """What `audio_from_spectrogram_images` returns of a rank's `result`, its clips' `errors` (None: not asked for) and the
        deferred range check's flag (None: nothing deferred)."""
        want_error = errors is not None
        if return_device:
            if range_ok is not None:
                # nothing on this path ever synchronises, so the deferred check cannot raise here: out-of-range (or NaN) input
                # yields SILENCE instead of garbage audio (one in-place multiply on the device, no host sync, no copy of the batch)
                result.mul_(range_ok.to(result.dtype))
            # the flag travels with the result for a caller that wants to look: `result.range_ok`, a 0-dim bool tensor on the device
            # (True when nothing was checked: uint8 input, validate=False, or a check that already ran on the host).  It is a plain
            # attribute: slicing / .to() / a gather make a new tensor without it - read it from the tensor this call returned.
            flag = range_ok if range_ok is not None else torch.ones((), dtype=torch.bool, device=result.device)
            result.range_ok = flag
            if want_error:
                return (result, errors, flag) if return_range_flag else (result, errors)
            return (result, flag) if return_range_flag else result
        if result.is_cuda:
            host = torch.empty(result.shape, dtype=result.dtype, pin_memory=True)  # gathered batch: one pinned copy
            host.copy_(result, non_blocking=True)
            torch.cuda.current_stream(plan.device).synchronize()
            result = host
        if range_ok is not None and not bool(range_ok):  # the stream has been synchronised above / by the sink: no extra wait
            raise ValueError(_RANGE_MSG)
        return (result.numpy(), errors.cpu().numpy()) if want_error else result.numpy()
