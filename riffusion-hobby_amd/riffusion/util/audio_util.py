"""
PCM container helpers.

`audio_from_waveform` keeps the reference's contract (riffusion/util/audio_util.py:13-36: joint
peak normalisation, truncation to int16, an `AudioSegment` back).  pydub is imported lazily: when it
is installed the functions return real `pydub.AudioSegment`s exactly like the reference; when it is
not (this image has no pydub) they return `PcmSegment`, a small stand-in that offers the part of the
AudioSegment interface the spectrogram path and its callers touch (frame_rate, channels,
sample_width, split_to_mono, get_array_of_samples, set_channels, set_frame_rate, duration_seconds,
rms / dBFS / max, apply_gain, append with crossfade, overlay, export to wav).  set_frame_rate has a restatement of its own (ratecv_np).

pydub.AudioSegment is a thin layer over CPython's `audioop` C module (mul, rms, max, tomono,
tostereo, ratecv, add).  `PcmSegment` calls the same `audioop` functions when the interpreter still
ships the module (Python <= 3.12; the reference pins 3.9), so its integer arithmetic IS the
reference's; the numpy restatements below it are used only where audioop is gone, and
tests/test_host_logic.py pins them against audioop bit for bit.  What remains from memory is
pydub 0.25.1's glue around those calls (which audioop function, which factor), cited per method.
"""
import functools
import io
import math
import typing as T

import numpy as np

try:  # the C module pydub itself calls; removed from CPython 3.13
    import audioop as _audioop  # type: ignore
except ImportError:  # pragma: no cover
    _audioop = None


def _pydub():
    try:
        import pydub  # type: ignore

        return pydub
    except ImportError:
        return None


class PcmSegment:
    """int16 PCM, (samples, channels) interleaved - the subset of pydub.AudioSegment this path needs."""

    sample_width = 2

    def __init__(self, samples: np.ndarray, frame_rate: int):
        samples = np.asarray(samples)
        if samples.ndim == 1:
            samples = samples[:, None]
        if samples.dtype != np.int16:
            raise TypeError("PcmSegment holds int16 samples")
        self._data = np.ascontiguousarray(samples)
        self.frame_rate = int(frame_rate)

    @property
    def channels(self) -> int:
        return int(self._data.shape[1])

    @property
    def duration_seconds(self) -> float:
        return self._data.shape[0] / float(self.frame_rate)

    def __len__(self) -> int:  # milliseconds, like pydub
        return int(round(1000.0 * self.duration_seconds))

    def frame_count(self) -> float:
        return float(self._data.shape[0])

    def get_array_of_samples(self) -> np.ndarray:
        return self._data.reshape(-1)

    def split_to_mono(self) -> T.List["PcmSegment"]:
        return [PcmSegment(self._data[:, c].copy(), self.frame_rate) for c in range(self.channels)]

    # ---- byte-level helpers ---------------------------------------------------------------------------------
    def _bytes(self) -> bytes:
        return self._data.tobytes()

    def _spawn(self, raw: bytes, channels: T.Optional[int] = None, frame_rate: T.Optional[int] = None) -> "PcmSegment":
        ch = self.channels if channels is None else channels
        return PcmSegment(np.frombuffer(raw, dtype=np.int16).reshape(-1, ch).copy(), self.frame_rate if frame_rate is None else frame_rate)

    @staticmethod
    def _mul_np(x: np.ndarray, factor: float) -> np.ndarray:
        """audioop.mul on int16: floor(clip(sample * factor)) with audioop's fbound (max 32767, min -32768)."""
        v = x.astype(np.float64) * float(factor)
        v = np.where(v > 32767.0, 32767.0, np.where(v < -32768.0, -32768.0, v))
        return np.floor(v).astype(np.int16)

    def set_channels(self, channels: int) -> "PcmSegment":
        """pydub AudioSegment.set_channels: mono -> stereo = audioop.tostereo(data, 2, 1, 1); stereo -> mono =
        audioop.tomono(data, 2, 0.5, 0.5)."""
        if channels == self.channels:
            return self
        if channels == 2 and self.channels == 1:
            if _audioop is not None:
                return self._spawn(_audioop.tostereo(self._bytes(), 2, 1, 1), channels=2)
            return PcmSegment(np.repeat(self._data, 2, axis=1), self.frame_rate)
        if channels == 1 and self.channels == 2:
            if _audioop is not None:
                return self._spawn(_audioop.tomono(self._bytes(), 2, 0.5, 0.5), channels=1)
            return PcmSegment(self._tomono_np(self._data), self.frame_rate)
        raise ValueError("PcmSegment.set_channels only converts between mono and stereo")

    @staticmethod
    def _tomono_np(x: np.ndarray) -> np.ndarray:
        """audioop.tomono(data, 2, 0.5, 0.5): floor(clip(l * 0.5 + r * 0.5)) in double."""
        v = x[:, 0].astype(np.float64) * 0.5 + x[:, 1].astype(np.float64) * 0.5
        return np.floor(np.clip(v, -32768.0, 32767.0)).astype(np.int16)

    def set_frame_rate(self, frame_rate: int) -> "PcmSegment":
        """pydub AudioSegment.set_frame_rate: audioop.ratecv(data, 2, channels, old, new, None) (linear
        interpolation resampler).  The reference's batch CLI calls it for files whose rate differs from the
        params' (cli.py:186-187)."""
        if int(frame_rate) == self.frame_rate:
            return self
        if _audioop is None:
            return PcmSegment(ratecv_np(self._data, self.frame_rate, int(frame_rate)), int(frame_rate))
        raw, _ = _audioop.ratecv(self._bytes(), 2, self.channels, self.frame_rate, int(frame_rate), None)
        return self._spawn(raw, frame_rate=int(frame_rate))

    # ---- the gain filters audio_util.apply_filters needs (pydub 0.25.1 AudioSegment.rms / dBFS / max /
    # apply_gain, effects.normalize) ---------------------------------------------------------------------
    max_possible_amplitude = 32768.0  # (2 ** 16) / 2

    @property
    def rms(self) -> int:
        """audioop.rms: floor(sqrt(sum(x^2) / n)) in double."""
        if _audioop is not None:
            return int(_audioop.rms(self._bytes(), 2))
        x = self._data.astype(np.float64).reshape(-1)
        return int(np.sqrt(np.sum(x * x) / x.size)) if x.size else 0

    @property
    def dBFS(self) -> float:
        """ratio_to_db(rms / max_possible_amplitude) = 20 * log(ratio, 10); -inf for silence."""
        import math

        rms = self.rms
        return float("-inf") if rms == 0 else 20.0 * math.log(rms / self.max_possible_amplitude, 10)

    @property
    def max(self) -> int:
        """audioop.max: largest absolute sample value."""
        if _audioop is not None:
            return int(_audioop.max(self._bytes(), 2))
        return int(np.abs(self._data.astype(np.int32)).max()) if self._data.size else 0

    def apply_gain(self, volume_change: float) -> "PcmSegment":
        """audioop.mul(data, 2, db_to_float(volume_change)), db_to_float(db) = 10 ** (db / 20)."""
        factor = 10 ** (float(volume_change) / 20)
        if _audioop is not None:
            return self._spawn(_audioop.mul(self._bytes(), 2, factor))
        return PcmSegment(self._mul_np(self._data, factor), self.frame_rate)

    def normalize(self, headroom: float = 0.1) -> "PcmSegment":
        """pydub.effects.normalize: boost so that the peak sits `headroom` dB below full scale."""
        import math

        peak = self.max
        if peak == 0:
            return self
        target_peak = self.max_possible_amplitude * (10 ** (-float(headroom) / 20))
        return self.apply_gain(20 * math.log(target_peak / peak, 10))

    def compress_dynamic_range(self, threshold: float = -20.0, ratio: float = 4.0, attack: float = 5.0,
                               release: float = 50.0) -> "PcmSegment":
        """pydub.effects.compress_dynamic_range (pydub 0.25.1), the same integers: the rms of the `look_frames` input frames
        before each frame (audioop.rms: exact int64 window sums, floor(sqrt(s / n)) in double), pydub's attenuation recurrence
        over the values tabulated by rms (compress_tables), and audioop.mul of each frame by 10 ** (-attenuation / 20)."""
        look, above, max_att, inc, dec = compress_tables(self.frame_rate, threshold, ratio, attack, release)
        att = compress_attenuation(compress_window_rms(self._data, look), above, max_att, inc, dec)
        return PcmSegment(compress_apply(self._data, att), self.frame_rate)

    # ---- joining clips (pydub AudioSegment.append / fade / overlay), used by stitch_segments / overlay_segments
    def _frames_of_ms(self, ms: float) -> int:
        return int(ms * (self.frame_rate / 1000.0))

    def _parse_position(self, val: float) -> int:
        """pydub AudioSegment._parse_position: milliseconds (negative = from the end, measured on the ROUNDED length in ms) -> frame index."""
        if val < 0:
            val = len(self) - abs(val)
        return int(self._frames_of_ms_f(len(self) if val == float("inf") else val))

    def _frames_of_ms_f(self, ms: float) -> float:
        return ms * (self.frame_rate / 1000.0)

    def _slice_ms(self, start_ms: T.Optional[float], end_ms: T.Optional[float]) -> "PcmSegment":
        """pydub AudioSegment.__getitem__(slice(start_ms, end_ms)): bounds clipped to len(self) - the length ROUNDED to whole
        milliseconds - so `seg[a:]` drops the frames past the last whole millisecond of a clip that is not a whole number of ms
        long, and a slice whose end lies past the data (the length rounded UP) is padded with silence (at most 2 ms, like pydub,
        which raises beyond that)."""
        length_ms = len(self)
        start = 0 if start_ms is None else min(start_ms, length_ms)
        end = length_ms if end_ms is None else min(end_ms, length_ms)
        a, b = self._parse_position(start), self._parse_position(end)
        data = self._data[a:b] if b > a else self._data[0:0]
        missing = max(0, b - a) - data.shape[0]
        if missing > 0:
            if missing > self._frames_of_ms_f(2):
                raise ValueError(f"slice is missing {missing} frames (pydub: TooManyMissingFrames)")
            data = np.concatenate([data, np.zeros((missing, self.channels), dtype=np.int16)])
        return PcmSegment(data, self.frame_rate)

    def _fade(self, to_gain: float = 0.0, from_gain: float = 0.0) -> "PcmSegment":
        """pydub AudioSegment.fade(to_gain, from_gain, start=0, end=inf), as append() calls it: the result is REBUILT from
        pieces - fades of more than 100 ms from the one-millisecond slices self[i] (gain stepped once per millisecond), shorter
        ones frame by frame - followed by self[len(self):], which is empty: frames past the last whole millisecond are dropped,
        exactly as pydub drops them.  Each step is an audioop.mul."""
        if to_gain == 0 and from_gain == 0:
            return self
        duration = len(self)
        from_power = 10 ** (float(from_gain) / 20)
        gain_delta = 10 ** (float(to_gain) / 20) - from_power
        mul = (lambda x, f: np.frombuffer(_audioop.mul(np.ascontiguousarray(x).tobytes(), 2, f), dtype=np.int16).reshape(x.shape)) \
            if _audioop is not None else self._mul_np
        pieces = []
        if duration > 100:
            scale_step = gain_delta / duration
            for i in range(duration):  # chunk i = self[i] = self[i : i + 1]
                pieces.append(mul(self._slice_ms(i, i + 1)._data, from_power + scale_step * i))
        else:
            fade_frames = self._frames_of_ms_f(duration)
            scale_step = gain_delta / fade_frames if fade_frames else 0.0
            for i in range(int(fade_frames)):
                pieces.append(mul(self._data[i : i + 1], from_power + scale_step * i))
        after = self._slice_ms(duration, None)._data  # self[end:] with end = len(self): empty
        pieces.append(mul(after, 10 ** (float(to_gain) / 20)) if to_gain != 0 else after)
        return PcmSegment(np.concatenate(pieces) if pieces else self._data[0:0], self.frame_rate)

    def overlay(self, other: "PcmSegment") -> "PcmSegment":
        """pydub AudioSegment.overlay(seg) at position 0 without looping: audioop.add over the overlap
        (saturating int16 sum); the result keeps this segment's length."""
        other = other.set_channels(self.channels).set_frame_rate(self.frame_rate)
        n = min(self._data.shape[0], other._data.shape[0])
        out = self._data.copy()
        if _audioop is not None:
            raw = _audioop.add(np.ascontiguousarray(self._data[:n]).tobytes(), np.ascontiguousarray(other._data[:n]).tobytes(), 2)
            out[:n] = np.frombuffer(raw, dtype=np.int16).reshape(n, self.channels)
        else:
            out[:n] = np.clip(self._data[:n].astype(np.int32) + other._data[:n].astype(np.int32), -32768, 32767).astype(np.int16)
        return PcmSegment(out, self.frame_rate)

    def append(self, seg: "PcmSegment", crossfade: int = 100) -> "PcmSegment":
        """pydub AudioSegment.append: the last `crossfade` ms of this segment faded to -120 dB are overlaid with the first
        `crossfade` ms of `seg` faded in from -120 dB."""
        seg = seg.set_channels(self.channels).set_frame_rate(self.frame_rate)
        if not crossfade:
            return PcmSegment(np.concatenate([self._data, seg._data]), self.frame_rate)
        if crossfade > len(self):
            raise ValueError(f"Crossfade is longer than the original AudioSegment ({crossfade}ms > {len(self)}ms)")
        if crossfade > len(seg):
            raise ValueError(f"Crossfade is longer than the appended AudioSegment ({crossfade}ms > {len(seg)}ms)")
        xf = self._slice_ms(-crossfade, None)._fade(to_gain=-120).overlay(seg._slice_ms(None, crossfade)._fade(from_gain=-120))
        return PcmSegment(
            np.concatenate([self._slice_ms(None, -crossfade)._data, xf._data, seg._slice_ms(crossfade, None)._data]), self.frame_rate
        )

    @classmethod
    def silent(cls, duration: float = 1000, frame_rate: int = 11025) -> "PcmSegment":
        """pydub AudioSegment.silent: int(frame_rate * (duration / 1000.0)) frames of mono silence (11025 Hz by default)."""
        return cls(np.zeros(int(frame_rate * (duration / 1000.0)), dtype=np.int16), frame_rate)

    def export(self, out_f: T.Any, format: str = "wav") -> T.Any:
        if format != "wav":
            raise NotImplementedError("PcmSegment exports wav only; install pydub + ffmpeg for other formats")
        from scipy.io import wavfile

        wavfile.write(out_f, self.frame_rate, self._data if self.channels > 1 else self._data[:, 0])
        return out_f

    @classmethod
    def from_wav(cls, path_or_file: T.Any) -> "PcmSegment":
        from scipy.io import wavfile

        rate, data = wavfile.read(path_or_file)
        if data.dtype != np.int16:
            raise NotImplementedError("only 16-bit PCM wav files are supported without pydub")
        return cls(data, rate)


def resample_waveform(waveform: T.Any, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                      resampling_method: str = "sinc_interp_hann", device: str = "cuda") -> T.Any:
    """
    (..., L) float waveform -> (..., ceil(new L / orig)) float32 on the GPU: torchaudio.functional.resample(waveform, orig_freq,
    new_freq, lowpass_filter_width, rolloff) - torchaudio.transforms.Resample - with its default Hann-windowed sinc, band-limited, as
    one HIP kernel over the taps inside the window (rfx_resample_sinc).  Leading dimensions are kept; an input on the CPU goes to
    `device`, one on a GPU stays where it is, and the result stays on the GPU.  orig_freq == new_freq returns the input's values.
    Only "sinc_interp_hann" is served: "sinc_interp_kaiser" raises ValueError.  No gradient.  (The int16 path of the encode,
    `ratecv_np` / rfx_pcm16_resample, is audioop's two-point interpolation and stays what pydub's set_frame_rate computes.)
    """
    import torch

    from riffusion import _hip

    _hip.check_resample_method(resampling_method)
    if not isinstance(waveform, torch.Tensor) or waveform.is_complex() or waveform.dim() < 1:
        raise ValueError("resample_waveform takes a real (..., samples) tensor")
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or int(orig_freq) < 1 or int(new_freq) < 1:
        raise ValueError(f"frequencies must be positive integers, got {orig_freq!r} -> {new_freq!r}")
    if torch.is_grad_enabled() and waveform.requires_grad:
        raise RuntimeError("resample_waveform: the resampler has no backward; detach the input, or run under torch.no_grad()")
    lead = waveform.shape[:-1]
    w = waveform.detach().reshape(-1, waveform.shape[-1])
    w = (w if w.device.type == "cuda" else w.to(_hip.resolve_device(device))).to(torch.float32)
    out = _hip.resample_sinc(w, int(orig_freq), int(new_freq), lowpass_filter_width, rolloff)
    return out.reshape(*lead, out.shape[-1])


RATECV_RATE_LIMIT = 1 << 20  # reduced rates (rate / gcd) below this: audioop's double division is then the exact quotient


def ratecv_frames(in_frames: int, in_rate: int, out_rate: int) -> int:
    """Frames audioop.ratecv(data, 2, C, in_rate, out_rate, None) returns for `in_frames` frames."""
    g = math.gcd(int(in_rate), int(out_rate))
    a, b = int(in_rate) // g, int(out_rate) // g
    return 0 if in_frames <= 0 else (int(in_frames) - 1) * b // a + 1


def ratecv_np(x: np.ndarray, in_rate: int, out_rate: int) -> np.ndarray:
    """audioop.ratecv(data, 2, C, in_rate, out_rate, None)[0] on (L, C) int16 frames, in closed form: with a = in_rate / g,
    b = out_rate / g, output k is emitted when n_k = 1 + ceil(k a / b) input frames are consumed, with audioop's counter at
    d_k = (n_k - 1) b - k a, and is trunc(((x[n_k - 2] << 16) d_k + (x[n_k - 1] << 16) (b - d_k)) / b) >> 16 (x[-1] = 0).  audioop
    divides in double; while b < 2^21 that is the integer quotient taken here, so reduced rates of 2^20 or more are refused
    (csrc/rfx_pcm_in_core.h states the same arithmetic for the device)."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    if x.dtype != np.int16:
        raise TypeError("ratecv_np resamples int16 frames")
    if int(in_rate) <= 0 or int(out_rate) <= 0:
        raise ValueError("sampling rate not > 0")  # audioop's message
    g = math.gcd(int(in_rate), int(out_rate))
    a, b = int(in_rate) // g, int(out_rate) // g
    if a >= RATECV_RATE_LIMIT or b >= RATECV_RATE_LIMIT:
        raise ValueError(f"reduced rates {a} -> {b} must stay below 2^20")
    L, C = x.shape
    K = ratecv_frames(L, in_rate, out_rate)
    if K == 0:
        return np.zeros((0, C), dtype=np.int16)
    k = np.arange(K, dtype=np.int64)
    n = 1 + (k * a + b - 1) // b
    d = ((n - 1) * b - k * a)[:, None]
    wide = np.concatenate([np.zeros((1, C), np.int64), x.astype(np.int64) << 16])  # wide[j + 1] = x[j] << 16
    num = wide[n - 1] * d + wide[n] * (b - d)
    q = np.where(num >= 0, num // b, -((-num) // b))  # truncation toward zero
    return (q >> 16).astype(np.int16)


class ClipRanges(T.NamedTuple):
    """clip_frame_ranges' answer.  `index`: positions in clip_start_times of the clips that lie wholly inside the track and are
    `frames` long, `starts` their first frames; `host_index`: the other clips (a slice that reaches the track's end, a length
    that the millisecond arithmetic makes one frame off) - slice_audio_into_clips builds those; `last_short`: the last clip
    takes the reference's silence branch (it is then in `host_index`)."""

    index: np.ndarray
    starts: np.ndarray
    frames: int
    host_index: np.ndarray
    last_short: bool


def clip_frame_ranges(segment_frames: int, frame_rate: int, clip_start_times: T.Sequence[float], clip_duration_s: float) -> ClipRanges:
    """The frames `slice_audio_into_clips` cuts, from lengths alone (as stitch_plan plans a stitch): clip i is
    PcmSegment._slice_ms(int(t_i * 1000), int(t_i * 1000) + int(clip_duration_s * 1000)) - bounds clipped to the track's length
    rounded to whole milliseconds, positions int(ms * (rate / 1000.0)) - and the last clip gets silence appended when
    int(its duration * 1000) falls short of the clip duration.  `frames` is the length of a clip that nothing cuts short,
    int(duration_ms * (rate / 1000.0)) for a start at 0 (220 500 for 5 s at 44.1 kHz)."""
    frames_total, rate = int(segment_frames), int(frame_rate)
    per_ms = rate / 1000.0
    length_ms = int(round(1000.0 * (frames_total / float(rate))))  # PcmSegment.__len__
    duration_ms = int(clip_duration_s * 1000)
    Lw = int(duration_ms * per_ms)
    n = len(clip_start_times)
    index, starts, host = [], [], []
    last_short = False
    for i, t in enumerate(clip_start_times):
        start_ms = int(t * 1000)
        lo, hi = min(start_ms, length_ms), min(start_ms + duration_ms, length_ms)
        a, b = int(lo * per_ms), int(hi * per_ms)
        whole = start_ms >= 0 and b > a and b <= frames_total and b - a == Lw and hi == start_ms + duration_ms
        if i == n - 1:
            got = max(0, b - a)  # with its padding
            if duration_ms - int((got / float(rate)) * 1000) > 0:
                last_short, whole = True, False
        if whole:
            index.append(i)
            starts.append(a)
        else:
            host.append(i)
    return ClipRanges(np.array(index, dtype=np.int64), np.array(starts, dtype=np.int64), Lw, np.array(host, dtype=np.int64), last_short)


def pcm16_from_waveform(samples: np.ndarray, normalize: bool = False) -> np.ndarray:
    """(channels, samples) float -> (samples, channels) int16 with the reference's arithmetic
    (audio_util.py:22-28): in-place scale by 32767 / max|x| over all channels, then truncation."""
    samples = np.array(samples, dtype=np.float32, copy=True)
    if normalize:
        # numpy 1.x evaluates python-int / float32-scalar in float64; the in-place multiply then
        # happens in float32.  Written out so that numpy 2's weak scalars give the same result.
        scale = np.float32(np.float64(np.iinfo(np.int16).max) / np.float64(np.max(np.abs(samples))))
        samples *= scale
    return np.ascontiguousarray(samples.transpose(1, 0).astype(np.int16))


def segment_from_pcm16(pcm: np.ndarray, sample_rate: int) -> T.Any:
    """(samples, channels) int16 -> pydub.AudioSegment when pydub exists, else PcmSegment."""
    pydub = _pydub()
    if pydub is None:
        return PcmSegment(pcm, sample_rate)
    from scipy.io import wavfile

    wav_bytes = io.BytesIO()
    wavfile.write(wav_bytes, sample_rate, pcm)
    wav_bytes.seek(0)
    return pydub.AudioSegment.from_wav(wav_bytes)


def audio_from_waveform(samples: np.ndarray, sample_rate: int, normalize: bool = False) -> T.Any:
    """(channels, samples) float array -> audio segment (reference audio_util.py:13-36)."""
    return segment_from_pcm16(pcm16_from_waveform(samples, normalize=normalize), sample_rate)


def apply_filters(segment: T.Any, compression: bool = False) -> T.Any:
    """Gain to -12 dBFS and peak normalisation with 0.1 dB headroom (reference audio_util.py:39-72): pydub /
    audioop integer filters on the host.  pydub segments go through pydub itself; PcmSegment carries a
    copy of the filters on the same audioop calls, compress_dynamic_range included (compression=True: normalize, gain to
    -10 dBFS and the compressor first)."""
    if isinstance(segment, PcmSegment):
        if compression:
            segment = segment.normalize(headroom=0.1)
            segment = segment.apply_gain(-10 - segment.dBFS)
            segment = segment.compress_dynamic_range(threshold=-20.0, ratio=4.0, attack=5.0, release=50.0)
        return segment.apply_gain(-12 - segment.dBFS).normalize(headroom=0.1)
    pydub = _pydub()
    if pydub is None:
        raise NotImplementedError("apply_filters on a foreign segment type needs pydub")
    if compression:
        segment = pydub.effects.normalize(segment, headroom=0.1)
        segment = segment.apply_gain(-10 - segment.dBFS)
        segment = pydub.effects.compress_dynamic_range(segment, threshold=-20.0, ratio=4.0, attack=5.0, release=50.0)
    segment = segment.apply_gain(-12 - segment.dBFS)
    return pydub.effects.normalize(segment, headroom=0.1)


def stitch_segments(segments: T.Sequence[T.Any], crossfade_s: float) -> T.Any:
    """Concatenate with a crossfade (reference audio_util.py:75-85); pydub segments or PcmSegments."""
    crossfade_ms = int(crossfade_s * 1000)
    out = segments[0]
    for seg in segments[1:]:
        out = out.append(seg, crossfade=crossfade_ms)
    return out


def clip_start_times(duration_s: float, clip_duration_s: float = 5.0, overlap_duration_s: float = 0.2,
                     start_time_s: float = 0.0, max_duration_s: float = 20.0) -> np.ndarray:
    """The clip start times (s) of the reference's audio-to-audio task (streamlit/tasks/audio_to_audio.py:94-101, with its
    defaults: 5 s clips overlapping by 0.2 s, the first 20 s of the track): `duration_s` is the track's `duration_seconds`."""
    duration = min(max_duration_s, duration_s - start_time_s)
    increment_s = clip_duration_s - overlap_duration_s
    return start_time_s + np.arange(0, duration - clip_duration_s, increment_s)


def slice_audio_into_clips(segment: T.Any, clip_start_times: T.Sequence[float], clip_duration_s: float) -> T.List[T.Any]:
    """
    The reference's slice_audio_into_clips (streamlit/tasks/audio_to_audio.py:396-416) on a PcmSegment or a pydub segment:
    clip i is segment[int(t_i * 1000) : int(t_i * 1000) + int(clip_duration_s * 1000)] in integer milliseconds, as the
    reference truncates them (the fourth start of np.arange(0, 20, 4.8) is 14 399 ms).  A full 5 s clip at 44.1 kHz holds
    220 500 frames.

    The last clip's silence branch is kept AS THE REFERENCE HAS IT (its own comment: "I don't think this is working properly"):
    a last clip shorter than the clip duration gets `append(AudioSegment.silent(silence_ms))` with append's default crossfade of
    100 ms, so less than 100 ms of missing audio raises append's ValueError, and more is crossfaded into the clip's end
    instead of being added after it.  This port reproduces that; it does not fix it.
    """
    pydub = None if isinstance(segment, PcmSegment) else _pydub()
    clips: T.List[T.Any] = []
    for i, clip_start_time_s in enumerate(clip_start_times):
        clip_start_time_ms = int(clip_start_time_s * 1000)
        clip_duration_ms = int(clip_duration_s * 1000)
        if pydub is None:
            clip = segment._slice_ms(clip_start_time_ms, clip_start_time_ms + clip_duration_ms)
        else:
            clip = segment[clip_start_time_ms : clip_start_time_ms + clip_duration_ms]
        if i == len(clip_start_times) - 1:
            silence_ms = clip_duration_ms - int(clip.duration_seconds * 1000)
            if silence_ms > 0:
                silence = PcmSegment.silent(duration=silence_ms) if pydub is None else pydub.AudioSegment.silent(duration=silence_ms)
                clip = clip.append(silence)
        clips.append(clip)
    return clips


# ---- the same two operations on the device (riffusion/_hip.py Plan.apply_filters / Plan.stitch, csrc/rfx_pcm.hip) -------------
# The device reproduces the audioop arithmetic above byte for byte.  What it cannot reproduce bit for bit - Python's pow and
# log - is tabulated here, and what is pydub's millisecond bookkeeping - the lengths of append's slices and fades - is planned
# here, from lengths alone.

FILTER_TABLE_SIZE = 32769  # audioop.rms and audioop.max of 16-bit samples lie in 0..32768
FILTER_EXACT_SAMPLES = 1 << 23  # the device filters equal audioop's while a clip holds fewer samples (L * C) than this


@functools.lru_cache(maxsize=None)
def filter_gain_by_rms(target: float = -12) -> np.ndarray:
    """Factor of apply_gain(target - dBFS) for every audioop.rms value, with PcmSegment's expressions (dBFS = -inf for rms 0:
    entry 0 is inf).  apply_filters uses -12, and -10 before the compressor."""
    out = np.empty(FILTER_TABLE_SIZE, dtype=np.float64)
    for rms in range(FILTER_TABLE_SIZE):
        dbfs = float("-inf") if rms == 0 else 20.0 * math.log(rms / PcmSegment.max_possible_amplitude, 10)
        out[rms] = 10 ** (float(target - dbfs) / 20)
    out.flags.writeable = False
    return out


# ---- compress_dynamic_range (pydub 0.25.1 effects.py), split at the one sequential part: every window rms is known before the
# loop (the windows read the compressor's input), so only the attenuation recurrence runs frame after frame.

@functools.lru_cache(maxsize=None)
def compress_tables(frame_rate: int, threshold: float = -20.0, ratio: float = 4.0, attack: float = 5.0,
                    release: float = 50.0) -> T.Tuple[int, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(look_frames, above, max_att, inc, dec) of compress_dynamic_range at this frame rate: for every audioop.rms value
    0..32768 of a window, pydub's own expressions - above = rms > thresh_rms, max_attenuation = (1 - 1 / ratio) *
    db_over_threshold(rms), and its per-frame attack increment and release decrement.  The device indexes these tables and
    evaluates no log."""
    thresh_rms = PcmSegment.max_possible_amplitude * (10 ** (float(threshold) / 20))  # max_possible_amplitude * db_to_float
    attack_frames = attack * (frame_rate / 1000.0)  # seg.frame_count(ms=attack)
    release_frames = release * (frame_rate / 1000.0)
    look_frames = int(attack_frames)
    above = np.zeros(FILTER_TABLE_SIZE, dtype=np.uint8)
    max_att, inc, dec = (np.empty(FILTER_TABLE_SIZE, dtype=np.float64) for _ in range(3))
    for rms in range(FILTER_TABLE_SIZE):
        if rms == 0:
            db_over = 0.0
        else:
            db = 20 * math.log(float(rms / thresh_rms), 10)  # ratio_to_db
            db_over = max(db, 0)
        m = (1 - (1.0 / ratio)) * db_over
        above[rms] = rms > thresh_rms
        max_att[rms], inc[rms], dec[rms] = m, m / attack_frames, m / release_frames
    for t in (above, max_att, inc, dec):
        t.flags.writeable = False
    return look_frames, above, max_att, inc, dec


def compress_window_rms(x: np.ndarray, look_frames: int) -> np.ndarray:
    """audioop.rms of seg.get_sample_slice(i - look_frames, i) for every frame i of an (L, C) int16 clip: frames
    [max(0, i - look), i), channels interleaved, 0 for an empty window.  The window sums are exact int64 prefix differences
    (audioop sums the squares in double, exact below 2^53)."""
    L, C = x.shape
    energy = (x.astype(np.int64) ** 2).sum(axis=1)
    prefix = np.zeros(L + 1, dtype=np.int64)
    np.cumsum(energy, out=prefix[1:])
    i = np.arange(L, dtype=np.int64)
    lo = np.maximum(i - look_frames, 0)
    n = (i - lo) * C
    s = (prefix[i] - prefix[lo]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = np.sqrt(s / n.astype(np.float64))
    return np.where(n > 0, rms, 0.0).astype(np.uint32)


def compress_attenuation(rms: np.ndarray, above: np.ndarray, max_att: np.ndarray, inc: np.ndarray, dec: np.ndarray) -> np.ndarray:
    """pydub's attenuation recurrence over the per-frame window rms values -> the attenuation after each frame (float64).
    Python's min / max: min(a, m) is a unless m < a, max(a, 0) is a unless 0 > a."""
    above_l, m_l, inc_l, dec_l = (above.astype(bool).tolist(), max_att.tolist(), inc.tolist(), dec.tolist())
    att = 0.0
    out = []
    append = out.append
    for r in rms.tolist():
        m = m_l[r]
        if above_l[r] and att <= m:
            att = att + inc_l[r]
            att = min(att, m)
        else:
            att = att - dec_l[r]
            att = max(att, 0)
        append(att)
    return np.array(out, dtype=np.float64)


def compress_apply(x: np.ndarray, att: np.ndarray) -> np.ndarray:
    """Each frame of an (L, C) int16 clip whose attenuation is not 0.0 -> audioop.mul(frame, 2, db_to_float(-attenuation)),
    the factor 10 ** (-attenuation / 20) evaluated by Python."""
    out = x.copy()
    idx = np.flatnonzero(att != 0.0)
    if idx.size == 0:
        return out
    factors = np.array([10 ** (float(-a) / 20) for a in att[idx].tolist()], dtype=np.float64)
    v = x[idx].astype(np.float64) * factors[:, None]
    v = np.where(v > 32767.0, 32767.0, np.where(v < -32768.0, -32768.0, v))
    out[idx] = np.floor(v).astype(np.int16)
    return out


@functools.lru_cache(maxsize=None)
def filter_boost_by_peak(headroom: float = 0.1) -> np.ndarray:
    """Factor of normalize(headroom) for every audioop.max value, with PcmSegment's expressions (a silent segment is returned
    unchanged: entry 0 is 1.0)."""
    out = np.empty(FILTER_TABLE_SIZE, dtype=np.float64)
    out[0] = 1.0
    target_peak = PcmSegment.max_possible_amplitude * (10 ** (-float(headroom) / 20))
    for peak in range(1, FILTER_TABLE_SIZE):
        out[peak] = 10 ** (float(20 * math.log(target_peak / peak, 10)) / 20)
    out.flags.writeable = False
    return out


# one piece of a stitched output: include/rfx.h rfx_stitch_piece (csrc/rfx_pcm_core.h PcmPiece)
STITCH_PIECE_DTYPE = np.dtype([("out_start", "<i8"), ("a_off", "<i8"), ("b_off", "<i8"), ("a_gain", "<f8"), ("b_gain", "<f8"),
                               ("a_clip", "<i4"), ("b_clip", "<i4"), ("kind", "<i4"), ("reserved", "<i4")])


class StitchNotPlannable(NotImplementedError):
    """A crossfade that reaches back into the previous crossfade (clips shorter than about two crossfades): the pieces of one
    pass cannot describe it."""


def stitch_plan(n_clips: int, frames: int, frame_rate: int, crossfade_s: float) -> T.Tuple[np.ndarray, int]:
    """
    `stitch_segments` of `n_clips` clips of `frames` frames each, planned from the lengths alone: the pieces the device stitch
    (rfx_pcm16_stitch) writes the output from, and the output's length in frames.  It follows PcmSegment.append step by step -
    lengths rounded to whole milliseconds, slices at int(ms * (rate / 1000.0)), frames past the last whole millisecond dropped,
    silence where a slice runs past the data, fades of more than 100 ms stepped once per millisecond and shorter ones once per
    frame - and every gain is evaluated here, with append's own `from_power + scale_step * i`.  Raises append's ValueError when
    the crossfade is longer than a clip, and StitchNotPlannable when a crossfade would read a previous one.
    """
    n_clips, frames, rate = int(n_clips), int(frames), int(frame_rate)
    if n_clips < 1 or frames < 1 or rate < 1:
        raise ValueError("stitch_plan needs at least one clip of at least one frame")
    crossfade = int(crossfade_s * 1000)
    if crossfade < 0:
        raise ValueError(f"crossfade must not be negative, got {crossfade_s}")
    per_ms = rate / 1000.0

    def len_ms(n: int) -> int:  # PcmSegment.__len__
        return int(round(1000.0 * (n / float(rate))))

    def pos(ms: int) -> int:  # PcmSegment._parse_position of a position in [0, len]
        return int(ms * per_ms)

    def check_missing(missing: int) -> None:  # PcmSegment._slice_ms
        if missing > 2 * per_ms:
            raise ValueError(f"slice is missing {missing} frames (pydub: TooManyMissingFrames)")

    def fade(n: int, from_gain: float, to_gain: float) -> T.Tuple[int, np.ndarray, np.ndarray]:
        """PcmSegment._fade of an n-frame slice: (output frames, first frame of each gain step, gain of each step)."""
        duration = len_ms(n)
        from_power = 10 ** (float(from_gain) / 20)
        gain_delta = 10 ** (float(to_gain) / 20) - from_power
        if duration > 100:
            scale_step = gain_delta / duration
            starts = (np.arange(duration, dtype=np.float64) * per_ms).astype(np.int64)
            for i in range(duration):  # each one-millisecond slice s[i:i+1] is padded with silence where it runs past the data
                check_missing(max(0, pos(i + 1) - pos(i)) - max(0, min(pos(i + 1), n) - pos(i)))
            return pos(duration), starts, from_power + scale_step * np.arange(duration, dtype=np.float64)
        fade_frames = duration * per_ms
        scale_step = gain_delta / fade_frames if fade_frames else 0.0
        count = min(int(fade_frames), n)  # s[i:i+1] past the data is empty here: no padding
        return count, np.arange(count, dtype=np.int64), from_power + scale_step * np.arange(count, dtype=np.float64)

    # the output so far: ("copy", start, length, clip, offset) runs (clip -1: silence) and ("fade", start, length, pieces) blocks
    out: T.List[T.Tuple[T.Any, ...]] = [("copy", 0, frames, 0, 0)]
    total = frames
    for k in range(1, n_clips):
        if not crossfade:
            out.append(("copy", total, frames, k, 0))
            total += frames
            continue
        A, A2 = len_ms(total), len_ms(frames)
        if crossfade > A:
            raise ValueError(f"Crossfade is longer than the original AudioSegment ({crossfade}ms > {A}ms)")
        if crossfade > A2:
            raise ValueError(f"Crossfade is longer than the appended AudioSegment ({crossfade}ms > {A2}ms)")
        b1, bA = pos(A - crossfade), pos(A)  # head = out[:b1]; fade-out slice s1 = out[b1:bA], silence past `total`
        n1 = max(0, bA - b1)
        check_missing(n1 - max(0, min(bA, total) - b1))
        cf, bA2 = pos(crossfade), pos(A2)  # fade-in slice s2 = seg[:cf]; tail = seg[cf:bA2]
        check_missing(cf - min(cf, frames))
        if bA2 > cf:
            check_missing((bA2 - cf) - max(0, min(bA2, frames) - cf))
        xo, starts_o, gains_o = fade(n1, 0, -120)
        xi, starts_i, gains_i = fade(cf, -120, 0)
        n = min(xo, xi)  # overlay: the fade-in is added over the first n frames, the result keeps the fade-out's length
        # the fade-out reads these runs of `out` (positions relative to b1)
        src_a: T.List[T.Tuple[int, int, int, int]] = []  # (first, length, clip, offset of that first frame)
        while out and out[-1][1] + out[-1][2] > b1:
            entry = out.pop()
            if entry[0] == "fade":
                raise StitchNotPlannable("a crossfade longer than half a clip reaches into the previous crossfade")
            _, start, length, clip, off = entry
            if start < b1:  # the head keeps the first part of this run
                out.append(("copy", start, b1 - start, clip, off))
                off, length, start = off + (b1 - start), length - (b1 - start), b1
            src_a.append((start - b1, length, clip, off))
        src_a.reverse()
        if xo:
            edges = [e for first, length, _, _ in src_a for e in (first, first + length)]
            bounds = [starts_o, starts_i[starts_i < n], np.array(edges + [n1, n, cf, frames], dtype=np.int64)]
            p0 = np.unique(np.concatenate(bounds))
            p0 = p0[(p0 >= 0) & (p0 < xo)]
            if not len(p0) or p0[0] != 0:
                p0 = np.concatenate([np.zeros(1, np.int64), p0])
            pieces = np.zeros(len(p0), dtype=STITCH_PIECE_DTYPE)
            pieces["out_start"] = b1 + p0
            pieces["kind"] = 1
            pieces["a_gain"] = gains_o[np.searchsorted(starts_o, p0, side="right") - 1]
            pieces["a_clip"] = -1
            for first, length, clip, off in src_a:  # s1[j] = out[b1 + j] while that exists, silence after
                sel = (p0 >= first) & (p0 < first + length) & (p0 < n1) & (clip >= 0)
                pieces["a_clip"][sel] = clip
                pieces["a_off"][sel] = off + (p0[sel] - first)
            inb = p0 < n
            if len(starts_i):
                pieces["b_gain"][inb] = gains_i[np.searchsorted(starts_i, p0[inb], side="right") - 1]
            has_b = inb & (p0 < min(cf, frames))  # s2[j] = seg[j], silence past the clip and past the slice
            pieces["b_clip"] = np.where(has_b, k, -1)
            pieces["b_off"] = np.where(has_b, p0, 0)
            out.append(("fade", b1, xo, pieces))
        total = b1 + xo
        if bA2 > cf:
            if min(bA2, frames) > cf:
                out.append(("copy", total, min(bA2, frames) - cf, k, cf))
            if bA2 > frames:
                out.append(("copy", total + max(0, frames - cf), bA2 - max(cf, frames), -1, 0))
            total += bA2 - cf
    parts = []
    for entry in out:
        if entry[0] == "fade":
            parts.append(entry[3])
        elif entry[2] > 0:
            piece = np.zeros(1, dtype=STITCH_PIECE_DTYPE)
            piece["out_start"], piece["a_clip"], piece["a_off"], piece["b_clip"] = entry[1], entry[3], entry[4], -1
            parts.append(piece)
    return np.concatenate(parts), total


def overlay_segments(segments: T.Sequence[T.Any]) -> T.Any:
    """Overlay segments on top of each other (reference audio_util.py:88-100)."""
    assert len(segments) > 0
    output: T.Any = None
    for segment in segments:
        output = segment if output is None else output.overlay(segment)
    return output
