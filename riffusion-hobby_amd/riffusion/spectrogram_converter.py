"""
Audio <-> mel-amplitude spectrograms on the MI355X.

Drop-in for the reference's `riffusion/spectrogram_converter.py:12-204`: same constructor, same
attributes (`p`, `device`, `spectrogram_func`, `inverse_spectrogram_func`, `mel_scaler`,
`inverse_mel_scaler`), same methods and tensor layouts.  The four torchaudio modules the reference
builds (:47-99) are replaced by callables that run hand-written HIP kernels through librfx.so:

    spectrogram_func          torchaudio.transforms.Spectrogram(power=None)  -> framed 17640-pt transform
    mel_scaler                torchaudio.transforms.MelScale                 -> fp32-MFMA GEMM
    inverse_mel_scaler        torchaudio.transforms.InverseMelScale (SGD)    -> banded on-chip SGD
    inverse_spectrogram_func  torchaudio.transforms.GriffinLim               -> fused per-frame iteration

The two torch-level methods fuse these pairs so the (B, n_stft, T) intermediates of the reference are
never materialised; the standalone callables exist for code that pokes at the members directly.
The three forward members are differentiable, as the reference's are: with an input that requires grad they route through
riffusion/_autograd.py and the gradient runs on the device; the inverse members and the loop encode are not.  `spectral_losses`
(not in the reference) is the spectral convergence / log-magnitude L1 pair fused with the transform, forward and backward, plain and loop.
Every call is re-entrant: the converter holds immutable constants only (plans are cached per
(params, device)), workspaces are checked out of the plan's arena per call (`_hip.WorkspaceArena`: two
threads never share one) - the reference shares one converter across a thread pool (cli.py:172-204).  There is no CPU implementation: on a machine without a GPU the constructor still
mirrors the reference's fallback warning, and any compute call raises.
"""
import functools
import typing as T
import warnings

import numpy as np
import torch

from riffusion import _autograd
from riffusion._decode import ClipExtras
from riffusion.spectrogram_params import SpectrogramParams
from riffusion.util import audio_util, torch_util


class _HipOp:
    """A callable member standing where the reference keeps a torchaudio nn.Module."""

    def __init__(self, owner: "SpectrogramConverter", fn: T.Callable[..., torch.Tensor], name: str):
        self._owner, self._fn, self._name = owner, fn, name

    def __call__(self, *args: T.Any, **kwargs: T.Any) -> torch.Tensor:
        return self._fn(*args, **kwargs)

    def to(self, device: T.Any) -> "_HipOp":  # nn.Module-style chaining used by the reference ctor
        return self

    def __repr__(self) -> str:
        return f"<rfx HIP op {self._name} on {self._owner.device}>"


def hold_rows(hold_frames: T.Any, n: int, frames: int) -> torch.Tensor:
    """`hold_frames` as the (n, 2) int32 host tensor of {head, tail} the library reads: a `(head, tail)` pair serves all n entries,
    an (n, 2) integer array or tensor gives each its own; values are clamped to [0, frames]."""
    h = torch.as_tensor(np.asarray(hold_frames) if not isinstance(hold_frames, torch.Tensor) else hold_frames).cpu()
    if h.is_floating_point() or h.is_complex() or h.dtype == torch.bool:
        raise ValueError(f"hold_frames must be integers, got {h.dtype}")
    if h.dim() == 1 and h.shape[0] == 2:
        h = h.reshape(1, 2).expand(n, 2)
    if h.dim() != 2 or tuple(h.shape) != (n, 2):
        raise ValueError(f"hold_frames must be a (head, tail) pair or ({n}, 2) integers, got {tuple(h.shape)}")
    return h.to(torch.int64).clamp(0, frames).to(torch.int32).contiguous()


def hold_mask_rows(hold_mask: T.Any, n: int, n_mels: int, frames: int) -> torch.Tensor:
    """`hold_mask` as the (n, n_mels, frames) uint8 tensor (nonzero = held, spectrogram orientation: band 0 first) the library
    expands to bins: one (n_mels, frames) array or tensor serves all n entries, an (n, n_mels, frames) one gives each its own.
    The tensor stays on the device it came on."""
    m = torch.as_tensor(np.ascontiguousarray(hold_mask) if isinstance(hold_mask, np.ndarray) else hold_mask)
    if m.is_complex():
        raise ValueError(f"hold_mask must be boolean or real, got {m.dtype}")
    if m.dim() == 2:
        m = m[None].expand(n, *m.shape)
    if tuple(m.shape) != (n, n_mels, frames):
        raise ValueError(f"hold_mask must be ({n_mels}, {frames}) or ({n}, {n_mels}, {frames}), got {tuple(m.shape)}")
    return (m != 0).to(torch.uint8)


# the combination rules (`_hip.check_call_rules`) in the words of the converters' arguments
CALL_WORDING = {
    "roles": {"hold_frames": "hold", "hold_mask": "hold_bins", "guide_segment": "guide", "guide_waveforms": "guide"},
    "peak_start": 'phase_start="peaks" does not go with {given}: the peak start needs no guide and holds nothing',
    "loop_holds": "loop together with hold_frames or hold_mask is not served",
    "two_starts": "guide and angles0 are two starts of Griffin-Lim: give one",
    "hold_needs_guide": "hold_frames needs a guide: the frames are held at the guide's phase",
    "bins_need_guide": "hold_mask needs a guide: the bins are held at the guide's phase",
    "bins_and_hold": "hold_frames together with hold_mask is not served: set the held frames' columns in the mask",
}


class SpectralLosses(T.NamedTuple):
    """what `SpectrogramConverter.spectral_losses` returns: (B,) float64 each; `log_magnitude` is None without a log floor"""

    convergence: torch.Tensor
    log_magnitude: T.Optional[torch.Tensor]


class LoopLengthError(ValueError):
    """a clip that is no whole loop at the params: not a whole number of hops, or shorter than n_fft"""


class SpectrogramConverter:
    def __init__(self, params: SpectrogramParams, device: str = "cuda", *, frame_engine: str = "auto"):
        """`frame_engine="chirp-z"` (not in the reference) runs parameter sets whose FFT length has a prime factor above 13 - which
        "auto" refuses with the library's reason - on the chirp-z engine; every other parameter set is planned as under "auto"."""
        self.p = params
        self.frame_engine = frame_engine
        self.device = torch_util.check_device(device)
        if device.lower().startswith("mps"):
            warnings.warn(
                "WARNING: MPS does not support audio operations, falling back to CPU for them",
                stacklevel=2,
            )
            self.device = "cpu"

        self.spectrogram_func = _HipOp(self, self._spectrogram, "Spectrogram(power=None)")
        self.inverse_spectrogram_func = _HipOp(self, self._griffinlim, "GriffinLim")
        self.mel_scaler = _HipOp(self, self._mel_scale, "MelScale")
        self.inverse_mel_scaler = _HipOp(self, self._inverse_mel_scale, "InverseMelScale")

    # ---- plan -------------------------------------------------------------------------------
    def _plan(self):
        from riffusion import _hip  # deferred: importing the package must work without the .so

        if not str(self.device).startswith("cuda"):
            raise RuntimeError(
                f"SpectrogramConverter(device={self.device!r}): this build runs on the MI355X only "
                "(HIP kernels through librfx.so); there is no CPU implementation"
            )
        return _hip.get_plan(self.p, self.device, frame_engine=self.frame_engine)

    @property
    def _channels_per_clip(self) -> int:
        return 2 if self.p.stereo else 1

    # ---- the four members, with the reference's tensor layouts ----------------------------------
    def _spectrogram(self, waveform: torch.Tensor) -> torch.Tensor:
        """(B, samples) -> (B, n_stft, T) complex64."""
        plan = self._plan()
        lead = waveform.shape[:-1]
        w = waveform.reshape(-1, waveform.shape[-1]).to(self.device)
        if _autograd.wants_grad(w):  # differentiable as torchaudio's Spectrogram is: the gradient runs on the device (riffusion/_autograd.py)
            spec = _autograd.stft(plan, w.to(torch.float32))
            return spec.reshape(*lead, plan.n_stft, spec.shape[-1])
        _, spec, Tn = plan.stft(w, want_mag=False, want_spec=True)
        return plan.unpack_complex(spec, w.shape[0], Tn).reshape(*lead, plan.n_stft, Tn)

    def _mel_scale(self, amplitudes: torch.Tensor) -> torch.Tensor:
        """(B, n_stft, T) -> (B, n_mels, T); standalone use only (the fused path never builds the input)."""
        plan = self._plan()
        lead = amplitudes.shape[:-2]
        x = amplitudes.reshape(-1, amplitudes.shape[-2], amplitudes.shape[-1]).to(self.device)
        if _autograd.wants_grad(x):
            return _autograd.mel_scale(plan, x.to(torch.float32)).reshape(*lead, plan.n_mels, x.shape[-1])
        return plan.mel_scale(x).reshape(*lead, plan.n_mels, x.shape[-1])

    def _inverse_mel_scale(
        self, melspec: torch.Tensor, *, spec0: T.Optional[torch.Tensor] = None, seed: T.Optional[int] = None, inverse_mel: str = "sgd"
    ) -> torch.Tensor:
        """(B, n_mels, T) -> (B, n_stft, T).  `inverse_mel="lstsq"` (not in the reference's member; torchaudio >= 2.1's InverseMelScale):
        the closed form relu(fb G^-1 mel) on the device, (..., n_mels, T) -> (..., n_stft, T) with leading dimensions as `mel_scaler`
        takes them.  No random start: `spec0` and `seed` are refused.  Differentiable as torchaudio's is: a `melspec` that requires
        grad gives a result with a grad_fn, the gradient runs on the device (riffusion/_autograd.py).  The default "sgd" is the
        iterative solver, which has no gradient."""
        from riffusion import _hip

        if _hip.check_inverse_mel(inverse_mel):
            if spec0 is not None or seed is not None:
                raise ValueError('inverse_mel="lstsq" has no random start: spec0 and seed do not go with it')
            plan = self._plan()
            plan.require_lstsq()
            lead = melspec.shape[:-2]
            x = melspec.reshape(-1, melspec.shape[-2], melspec.shape[-1]).to(self.device)
            return _autograd.inverse_mel_lstsq(plan, x.to(torch.float32)).reshape(*lead, plan.n_stft, x.shape[-1])
        plan = self._plan()
        B, _, Tn = melspec.shape
        spec0 = spec0.to(self.device) if spec0 is not None else None
        slots = plan.inverse_mel(melspec.to(self.device), B, spec0=spec0, seed=self._seed(seed))
        return plan.unpack_magnitudes(slots, B, Tn)

    def _griffinlim(
        self, specgram: torch.Tensor, *, angles0: T.Optional[torch.Tensor] = None, seed: T.Optional[int] = None
    ) -> torch.Tensor:
        """(B, n_stft, T) magnitudes -> (B, hop*(T-1))."""
        plan = self._plan()
        B, _, Tn = specgram.shape
        slots = plan.pack_magnitudes(specgram.to(self.device))
        a0 = plan.pack_complex(angles0.to(self.device)) if angles0 is not None else None
        return plan.griffinlim(slots, B, Tn, self.p.num_griffin_lim_iters, 0.99, angles0_slots=a0, seed=self._seed(seed))

    @staticmethod
    def _seed(seed: T.Optional[int]) -> int:
        # the reference draws from torch's global generator (no seed parameter exists in its API):
        # derive ours from the same generator so torch.manual_seed() controls reproducibility
        if seed is not None:
            return int(seed)
        return int(torch.randint(0, 2**62, (1,)).item())

    # ---- numpy / pydub level (reference :101-163) -------------------------------------------------
    def check_loop_samples(self, samples: int) -> None:
        """ValueError for a clip of `samples` samples that is no whole loop at these params - a loop encode takes exactly hop * T
        samples, hop * T >= n_fft, and trims or pads nothing - naming the nearest lengths that are, in samples and milliseconds."""
        from riffusion import _hip

        try:
            _hip.check_loop_samples(self.p.hop_length, self.p.n_fft, samples)  # the library's rule decides
        except ValueError:
            hop, rate = self.p.hop_length, self.p.sample_rate
            below, above = _hip.loop_nearest_samples(hop, self.p.n_fft, samples)

            def ms(n: int) -> str:
                return f"{n} samples ({n * 1000.0 / rate:.3f} ms)"

            raise LoopLengthError(f"a loop clip is a whole number of hops (hop_length {hop}), at least n_fft = {self.p.n_fft} samples: got {ms(int(samples))}; "
                                  f"the nearest legal lengths are {ms(below) if below else 'none'} below and {ms(above)} above; nothing is trimmed or "
                                  "padded") from None

    def spectrogram_from_audio(self, audio: T.Any, loop: bool = False) -> np.ndarray:
        """Audio segment -> (channels, n_mels, T) float32 mel amplitudes.  `loop`: the segment is one period of a loop - exactly
        hop * T samples (`check_loop_samples`) - and is encoded on the circular STFT (`mel_amplitudes_from_waveform`): T columns."""
        assert int(audio.frame_rate) == self.p.sample_rate, "Audio sample rate must match params"
        waveform = np.array([c.get_array_of_samples() for c in audio.split_to_mono()])
        if waveform.dtype != np.float32:
            waveform = waveform.astype(np.float32)
        if loop:
            self.check_loop_samples(waveform.shape[-1])
        waveform_tensor = torch.from_numpy(waveform).to(self.device)
        amplitudes_mel = self.mel_amplitudes_from_waveform(waveform_tensor, loop=loop)
        return amplitudes_mel.cpu().numpy()

    def audio_from_spectrogram(self, spectrogram: np.ndarray, apply_filters: bool = True, *, loop: bool = False,
                               phase_start: str = "random") -> T.Any:
        """(channels, n_mels, T) mel amplitudes -> audio segment with that many channels.  `loop`: a loop decode
        (`waveform_from_mel_amplitudes`): hop*T samples whose end runs into their start.  `phase_start`: "random" (the reference) or
        "peaks", Griffin-Lim's start built from the magnitudes (`waveform_from_mel_amplitudes`)."""
        from riffusion import _hip

        peaks = _hip.check_phase_start(phase_start)
        amplitudes_mel = torch.from_numpy(np.ascontiguousarray(spectrogram)).to(self.device)
        plan = self._plan()
        waveform = self._waveform_from_mel(plan, amplitudes_mel, ClipExtras(loop=loop, peak_start=peaks))
        # peak-normalise + int16 truncation on the device (audio_util.py:22-28), one D2H of int16
        pcm, _ = plan.pcm16(waveform, channels=waveform.shape[0], normalize=True)
        host_filters = apply_filters and pcm.shape[1] * pcm.shape[2] >= audio_util.FILTER_EXACT_SAMPLES
        if apply_filters and not host_filters:  # audio_util.apply_filters on the device, same bytes (rfx_pcm16_apply_filters)
            plan.apply_filters(pcm, out=pcm)
        segment = audio_util.segment_from_pcm16(pcm[0].cpu().numpy(), self.p.sample_rate)
        if host_filters:  # a clip of 2^23 samples or more: audioop's double sum of squares is no longer exact to mirror
            segment = audio_util.apply_filters(segment, compression=False)
        return segment

    # ---- torch level seam (reference :165-204) ----------------------------------------------------
    def mel_amplitudes_from_waveform(self, waveform: torch.Tensor, loop: bool = False) -> torch.Tensor:
        """(B, samples) -> (B, n_mels, T): framed transform, magnitude and mel GEMM without leaving the GPU.
        `loop`: every row is one period of a loop, exactly hop * T samples with hop * T >= n_fft (any other length raises
        ValueError with the nearest legal lengths): the STFT is the circular one a loop decode runs - frame t, element i reads
        sample (hop t + i - n_fft // 2) mod (hop T) - so the tile has T columns, closes at the loop point, and a loop decode's
        output gives its T frames back.  Columns whose window lies inside the clip are bit for bit the plain encode's.
        Differentiable, as the reference's three forward modules are: when grad mode is on and `waveform` requires grad the result
        carries a grad_fn whose backward runs on the device (rfx_mel_from_waveform_backward; only the waveform is saved, and a CPU
        leaf's copy to the device is autograd's own).  The same bytes come out either way.  The loop encode has no backward yet:
        `loop=True` on a waveform that requires grad raises RuntimeError instead of returning a constant."""
        if loop:
            self.check_loop_samples(int(waveform.shape[-1]))
        if _autograd.wants_grad(waveform):
            if loop:
                raise RuntimeError("mel_amplitudes_from_waveform(loop=True): the loop encode has no backward yet; detach the waveform, "
                                   "or encode without loop to differentiate")
            return _autograd.mel_from_waveform(self._plan(), waveform.to(self.device).to(torch.float32))
        return self._plan().mel_from_waveform(waveform.to(self.device), loop=loop)

    def waveform_from_mel_amplitudes(
        self,
        amplitudes_mel: torch.Tensor,
        *,
        spec0: T.Optional[torch.Tensor] = None,
        angles0: T.Optional[torch.Tensor] = None,
        seed: T.Optional[int] = None,
        channels_per_clip: T.Optional[int] = None,
        inverse_mel: str = "sgd",
        guide: T.Optional[torch.Tensor] = None,
        hold_frames: T.Any = None,
        hold_mask: T.Any = None,
        loop: bool = False,
        phase_start: str = "random",
        griffin_lim_iters: T.Optional[int] = None,
    ) -> torch.Tensor:
        """
        (B, n_mels, T) -> (B, hop*(T-1)).  The reference treats the whole batch as ONE clip (the SGD
        loss mean couples its rows); `channels_per_clip` lets batched callers say how many consecutive
        rows form a clip (default: all of them, like the reference).  `spec0` (B, T, n_stft) and
        `angles0` (B, n_stft, T) inject the two random initialisations (tests); otherwise they are drawn
        on the device from `seed` / torch's global generator.
        `inverse_mel="lstsq"` takes torchaudio >= 2.1's InverseMelScale - relu of the minimum-norm least-squares solution, in
        closed form on the device (rfx_inverse_mel_lstsq) - in place of the SGD: no random start (`spec0` is refused), no
        coupling of rows; a bank it does not serve raises ValueError with the library's reason.
        `guide`: (B, Lg) float32 waveforms, any units; Griffin-Lim starts every row from the phase of its guide's STFT (the row
        cut or zero-padded at its end to hop*(T-1) samples) instead of random phases - in an audio-to-audio workflow the source
        clip, whose phase is nearly right already.  No randomness is left in Griffin-Lim then; a silent guide row gives a silent
        row.  Not together with `angles0`: they are two starts.
        `hold_frames`: with a guide, a `(head, tail)` pair for all rows or a (B, 2) integer array or tensor: the first `head` and
        the last `tail` frames of a row keep the guide's phase through every iteration instead of only starting from it
        (rfx_held_call_options) - the part of a clip that is known audio does not move.  `hold_frames_for` turns seconds of known
        audio into the pair.  Values are clamped to the frame count.
        `hold_mask`: with a guide and without `hold_frames`, a (B, n_mels, T) boolean (or nonzero = held) array or tensor in the
        layout of the mel tensor: the linear bins every one of whose mel bands is held at a frame keep the guide's phase there
        through every iteration (rfx_masked_call_options) - the kept region of a partial regeneration under a mask image.
        `loop`: the T columns are one period of a loop (rfx_loop_call_options): Griffin-Lim runs on the circular STFT, the result
        has hop*T samples and its end runs into its start - no click when the clip is played on repeat.  T must reach n_fft / hop
        (40 at the defaults); not together with `hold_frames` or `hold_mask`.
        `phase_start`: "random" (the reference's U[0,1) start) or "peaks": Griffin-Lim starts from phases built from the linear
        magnitudes alone - the spectral peaks of every frame, their interpolated frequencies integrated over the hop
        (rfx_start_call_options).  No guide and no randomness in Griffin-Lim; it needs fewer iterations for the same spectral
        convergence at low iteration counts (README).  Not together with `angles0`, `guide`, `hold_frames` or `hold_mask`.
        `griffin_lim_iters`: Griffin-Lim iterations in place of the params' count (None), as `audio_from_spectrogram_images` has it.
        Differentiable in ONE form, the guided decode as a layer: with grad mode on and an `amplitudes_mel` that requires grad, the
        call with `inverse_mel="lstsq"`, a `guide`, `griffin_lim_iters=0` and no `hold_frames`, `hold_mask`, `spec0` or `angles0`
        (`loop` allowed) returns ISTFT(relu(lstsq(mel)) a / |a|), a = STFT(guide), with a grad_fn whose backward runs on the device
        in slot layout from end to end (rfx_waveform_from_mel_guided_backward; `mel` and the guide are saved, the guide is analysed
        again; a double backward raises).  The guide is a constant: one that requires grad raises.  Leading dimensions -
        (..., n_mels, T) with a (..., Lg) guide - and a CPU leaf are handled as `inverse_mel_scaler` handles them.  Every other call
        is the plain call, without a graph: Griffin-Lim iterations, the SGD and the held and masked forms have no gradient.
        """
        from riffusion import _hip

        if griffin_lim_iters is not None and (int(griffin_lim_iters) != griffin_lim_iters or int(griffin_lim_iters) < 0):
            raise ValueError(f"griffin_lim_iters must be a non-negative integer or None, got {griffin_lim_iters!r}")
        peaks = _hip.check_phase_start(phase_start)
        rules = functools.partial(_hip.check_call_rules, CALL_WORDING, loop=loop, peak_start=peaks, angles0=angles0, guide=guide,
                                  hold_frames=hold_frames, hold_mask=hold_mask)
        rules("peak_start", "loop_holds", "two_starts", "hold_needs_guide")
        B, n_mels, frames = int(amplitudes_mel.shape[0]), int(amplitudes_mel.shape[1]), int(amplitudes_mel.shape[-1])
        hold = hold_rows(hold_frames, B, frames) if hold_frames is not None else None
        rules("bins_need_guide", "bins_and_hold")
        bands = hold_mask_rows(hold_mask, B, n_mels, frames) if hold_mask is not None else None
        n_iter = self.p.num_griffin_lim_iters if griffin_lim_iters is None else int(griffin_lim_iters)
        if (_autograd.wants_grad(amplitudes_mel) and _hip.check_inverse_mel(inverse_mel) and guide is not None and n_iter == 0 and hold is None
                and bands is None and spec0 is None and angles0 is None):
            return self._guided_decode(amplitudes_mel, guide, seed, loop)
        clips = ClipExtras(guides=guide, holds=hold, bands=bands, loop=loop, peak_start=peaks, inverse_mel=inverse_mel, n_iter=n_iter)
        return self._waveform_from_mel(self._plan(), amplitudes_mel, clips, spec0=spec0, angles0=angles0, seed=seed, channels_per_clip=channels_per_clip)

    def _guided_decode(self, amplitudes_mel: torch.Tensor, guide: torch.Tensor, seed: T.Optional[int], loop: bool) -> torch.Tensor:
        """the differentiable form of `waveform_from_mel_amplitudes`: (..., n_mels, T) mel that requires grad, (..., Lg) guide"""
        from riffusion import _hip

        plan = self._plan()
        plan.require_lstsq()
        if amplitudes_mel.dim() < 3 or guide.dim() != amplitudes_mel.dim() - 1 or tuple(guide.shape[:-1]) != tuple(amplitudes_mel.shape[:-2]):
            raise ValueError(f"expected (..., n_mels, T) mel amplitudes and a (..., Lg) guide with the same leading dimensions, got "
                             f"{tuple(amplitudes_mel.shape)} and {tuple(guide.shape)}")
        if loop:
            _hip.check_loop_frames(self.p.hop_length, self.p.n_fft, int(amplitudes_mel.shape[-1]))
        lead = amplitudes_mel.shape[:-2]
        mel = amplitudes_mel.reshape(-1, amplitudes_mel.shape[-2], amplitudes_mel.shape[-1]).to(self.device).to(torch.float32)
        g = guide.reshape(-1, guide.shape[-1]).to(self.device, torch.float32)
        wave = _autograd.guided_decode(plan, mel, g, loop, self._seed(seed))
        return wave.reshape(*lead, wave.shape[-1])

    def hold_frames_for(self, head_s: float = 0.0, tail_s: float = 0.0) -> T.Tuple[int, int]:
        """`SpectrogramParams.hold_frames_for` of this converter's params: the `hold_frames` pair for `head_s` / `tail_s` seconds
        of known audio at a clip's two ends."""
        return self.p.hold_frames_for(head_s, tail_s)

    def _waveform_from_mel(self, plan: T.Any, amplitudes_mel: torch.Tensor, clips: ClipExtras = ClipExtras(), *,
                           tiles: T.Optional[T.Tuple[int, int, int]] = None, spec0: T.Optional[torch.Tensor] = None,
                           angles0: T.Optional[torch.Tensor] = None, seed: T.Optional[int] = None,
                           channels_per_clip: T.Optional[int] = None, row_base: int = 0, magnitude_hint: float = 0.0,
                           return_slots: bool = False) -> T.Any:
        """`waveform_from_mel_amplitudes` on a plan the caller already holds (the batch entry points fetch it once per call,
        not once per chunk and stage: a fetch is a lock and a dictionary lookup, and after an eviction a rebuild).
        `return_slots=True` runs the two inverse stages separately - same bits as the one call - and returns
        (waveform, linear magnitudes in slot layout): what `Plan.spectral_error` compares.  `clips`: the call's guides, holds,
        bands, flags and iterations, whose combination the caller has checked; `tiles=(a, b, C)`: the rows are the C channel rows
        of its clips [a, b) (`ClipExtras.rows`), None: its entries are the rows."""
        from riffusion import _hip

        if clips.loop:
            _hip.check_loop_frames(self.p.hop_length, self.p.n_fft, int(amplitudes_mel.shape[-1]))

        lstsq = _hip.check_inverse_mel(clips.inverse_mel)
        if lstsq:
            if spec0 is not None:
                raise ValueError('inverse_mel="lstsq" has no random start: spec0 does not go with it')
            plan.require_lstsq()
        mel = amplitudes_mel.to(self.device)
        B, _, Tn = mel.shape
        cpc = B if channels_per_clip is None else channels_per_clip
        s = self._seed(seed)
        n_iter = self.p.num_griffin_lim_iters if clips.n_iter is None else int(clips.n_iter)
        extras = clips.rows(plan, tiles)
        if spec0 is None and angles0 is None and not return_slots:  # the production path: one call (rfx_waveform_from_mel), same bits as the two below
            return plan.waveform_from_mel(mel, cpc, n_iter, 0.99, seed=s, row_base=row_base, magnitude_hint=magnitude_hint, extras=extras)
        spec0 = spec0.to(self.device) if spec0 is not None else None
        if lstsq:
            lin_slots = plan.inverse_mel_lstsq(mel)
        else:
            lin_slots = plan.inverse_mel(mel, cpc, spec0=spec0, seed=s, row_base=row_base, magnitude_hint=magnitude_hint)
        a0 = plan.pack_complex(angles0.to(self.device)) if angles0 is not None else None
        wave = plan.griffinlim(lin_slots, B, Tn, n_iter, 0.99, angles0_slots=a0, seed=s + 1, row_base=row_base, magnitude_hint=magnitude_hint, extras=extras)
        return (wave, lin_slots) if return_slots else wave

    # ---- inverse spectrogram: complex STFT -> audio ----------------------------------------------------
    def waveform_from_spectrogram(self, spec: torch.Tensor, length: T.Optional[int] = None, loop: bool = False) -> torch.Tensor:
        """
        (..., n_stft, T) complex64 -> (..., L) float32: torchaudio.transforms.InverseSpectrogram at this converter's parameters, the
        way back from `spectrogram_func` - torch.istft(center=True) on the device (rfx_istft), L = hop * (T - 1) (+ 1 for an odd
        n_fft).  For code that edits the complex spectrum - a time-frequency mask, a separator's ratio mask, bins spliced from
        another source - and for models that predict STFT coefficients.  Leading dimensions and a CPU input are handled as
        `spectrogram_func` handles them.
        `length`: the result is cut, or zero-padded at its end, to that many samples with torch operations, so autograd composes.
        A cut is torch.istft(length=)'s; past L torch keeps up to n_fft // 2 samples of its untrimmed tail, this member pads zeros.
        `loop`: the T columns are one period of a loop and the synthesis is the circular one of a loop decode: hop * T samples
        whose end runs into their start; T must reach n_fft / hop.  The inverse of `Plan.stft(loop=True)`.
        Differentiable: with grad mode on and a `spec` that requires grad the result carries a grad_fn whose backward runs on the
        device (rfx_istft_backward: the synthesis is linear, nothing is saved, the gradient is its adjoint); a double backward
        raises.  Otherwise the forward call alone runs.  `inverse_spectrogram_func` stays Griffin-Lim, on magnitudes, without a
        gradient.
        """
        if not isinstance(spec, torch.Tensor) or not spec.is_complex():
            raise ValueError("waveform_from_spectrogram takes a complex (..., n_stft, T) spectrogram; magnitudes go to inverse_spectrogram_func")
        if spec.dim() < 2:
            raise ValueError(f"waveform_from_spectrogram takes (..., n_stft, T), got {tuple(spec.shape)}")
        n_stft = self.p.n_fft // 2 + 1
        if int(spec.shape[-2]) != n_stft:
            raise ValueError(f"expected {n_stft} linear bins, got {int(spec.shape[-2])}")
        if int(spec.shape[-1]) < 1:
            raise ValueError("waveform_from_spectrogram: no frames")
        if length is not None and (int(length) != length or int(length) < 0):
            raise ValueError(f"length must be a non-negative integer, got {length!r}")
        plan = self._plan()
        lead = spec.shape[:-2]
        x = spec.reshape(-1, spec.shape[-2], spec.shape[-1]).to(self.device).to(torch.complex64)
        wave = _autograd.istft(plan, x, loop)
        if length is not None:
            L = int(wave.shape[-1])
            wave = wave[:, : int(length)] if int(length) <= L else torch.nn.functional.pad(wave, (0, int(length) - L))
        return wave.reshape(*lead, wave.shape[-1])

    # ---- time stretch: the phase vocoder between the STFT and its inverse ------------------------------------
    def _check_stretch(self, what: str, x: T.Any, rate: T.Any) -> float:
        """the checks the two time-stretch members share, all before the plan is used: one finite positive rate, and no gradient"""
        from riffusion import _hip

        rate = _hip.check_stretch_rate(rate)
        if isinstance(x, torch.Tensor) and _autograd.wants_grad(x):
            raise RuntimeError(f"{what}: the time stretch has no backward; detach the input, or run under torch.no_grad()")
        return rate

    def time_stretch_spectrogram(self, spec: torch.Tensor, rate: float) -> torch.Tensor:
        """
        (..., n_stft, T) complex64 -> (..., n_stft, ceil(T / rate)) complex64: what
        torchaudio.transforms.TimeStretch(hop_length, n_freq=n_stft)(spec, rate) returns - torchaudio.functional.phase_vocoder on the
        device (rfx_phase_vocoder).  rate > 1 is faster and shorter, rate < 1 slower and longer; rate == 1 returns the input's
        values.  Phases are carried as wrapped turns with each bin's advance an exact fraction, so the result does not lose accuracy
        with T the way the float32 sum of absolute phase does.  One rate per call.  No gradient: a `spec` that requires grad while
        grad mode is on raises before any device work.  No loop form: the accumulated phase does not close over a period.
        """
        rate = self._check_stretch("time_stretch_spectrogram", spec, rate)
        if not isinstance(spec, torch.Tensor) or not spec.is_complex():
            raise ValueError("time_stretch_spectrogram takes a complex (..., n_stft, T) spectrogram")
        if spec.dim() < 2:
            raise ValueError(f"time_stretch_spectrogram takes (..., n_stft, T), got {tuple(spec.shape)}")
        n_stft = self.p.n_fft // 2 + 1
        if int(spec.shape[-2]) != n_stft:
            raise ValueError(f"expected {n_stft} linear bins, got {int(spec.shape[-2])}")
        if int(spec.shape[-1]) < 1:
            raise ValueError("time_stretch_spectrogram: no frames")
        plan = self._plan()
        lead = spec.shape[:-2]
        x = spec.detach().reshape(-1, spec.shape[-2], spec.shape[-1]).to(self.device).to(torch.complex64)
        B, _, Tn = x.shape
        out, Tout = plan.phase_vocoder(plan.pack_complex(x), B, Tn, rate)
        return plan.unpack_complex(out, B, Tout).reshape(*lead, n_stft, Tout)

    def time_stretch(self, waveform: torch.Tensor, rate: float, length: T.Optional[int] = None) -> torch.Tensor:
        """
        (..., samples) float32 -> (..., L) float32, the clip played `rate` times as fast at the same pitch: `spectrogram_func`, the
        phase vocoder and `waveform_from_spectrogram` in one call on the device (rfx_time_stretch), without the two layout passes the
        composition pays.  L = hop * (T_out - 1) (+ 1 for an odd n_fft) with T_out = ceil(T / rate) of the clip's T frames; `length`
        cuts the result or pads it with zeros at its end, as `waveform_from_spectrogram` does.  To match a clip generated at one
        tempo to another: rate = bpm_to / bpm_from.  One rate per call, no gradient, no loop form (see `time_stretch_spectrogram`):
        a stretched loop does not close at its loop point.
        """
        rate = self._check_stretch("time_stretch", waveform, rate)
        if not isinstance(waveform, torch.Tensor) or waveform.is_complex() or waveform.dim() < 1:
            raise ValueError("time_stretch takes a real (..., samples) waveform")
        if length is not None and (int(length) != length or int(length) < 0):
            raise ValueError(f"length must be a non-negative integer, got {length!r}")
        plan = self._plan()
        lead = waveform.shape[:-1]
        w = waveform.detach().reshape(-1, waveform.shape[-1]).to(self.device).to(torch.float32)
        wave = plan.time_stretch(w, rate)
        if length is not None:
            L = int(wave.shape[-1])
            wave = wave[:, : int(length)] if int(length) <= L else torch.nn.functional.pad(wave, (0, int(length) - L))
        return wave.reshape(*lead, wave.shape[-1])

    # ---- pitch shift: the time stretch, then the resampler back to the duration -----------------------------
    def pitch_shift(self, waveform: torch.Tensor, n_steps: float, bins_per_octave: int = 12) -> torch.Tensor:
        """
        (..., samples) float32 -> (..., samples) float32, the clip moved by `n_steps` steps of 1 / `bins_per_octave` octave at the same
        tempo: what torchaudio.transforms.PitchShift(sample_rate, n_steps, bins_per_octave, n_fft, win_length, hop_length)(waveform)
        computes at the converter's own STFT parameters, in one call on the device (rfx_pitch_shift): `time_stretch` at rate
        2^(-n_steps / bins_per_octave), cut or zero-padded to round(samples / rate), the windowed-sinc resampler from
        int(sample_rate / rate) back to sample_rate, cut or zero-padded to `samples`.  +12 is an octave up, -12 an octave down;
        n_steps == 0 returns the input's values.  To put a generated clip in the key of the clip it is stitched to, shift it
        by the difference in semitones.
        One departure from torchaudio: where round(samples / rate) exceeds the stretched clip's hop * (T_out - 1) samples - by less
        than one hop - torch.istft(length=) keeps samples of its untrimmed tail and this call pads zeros, as `waveform_from_spectrogram(
        length=)` does.  With o / n the reduced pair int(sample_rate / rate) / sample_rate this reaches at most the last
        ceil((round(samples / rate) - hop * (T_out - 1)) * n / o + 6 * n / (0.99 * min(o, n))) + 1 output samples.
        One shift per call, no gradient (a `waveform` that requires grad while grad mode is on raises before any device work), no
        loop form, for the reasons `time_stretch` gives.
        """
        from riffusion import _hip

        n_steps, bins_per_octave = _hip.check_pitch_steps(n_steps, bins_per_octave)
        if isinstance(waveform, torch.Tensor) and _autograd.wants_grad(waveform):
            raise RuntimeError("pitch_shift: the pitch shift has no backward; detach the input, or run under torch.no_grad()")
        if not isinstance(waveform, torch.Tensor) or waveform.is_complex() or waveform.dim() < 1:
            raise ValueError("pitch_shift takes a real (..., samples) waveform")
        plan = self._plan()
        lead = waveform.shape[:-1]
        w = waveform.detach().reshape(-1, waveform.shape[-1]).to(self.device).to(torch.float32)
        return plan.pitch_shift(w, n_steps, bins_per_octave).reshape(*lead, waveform.shape[-1])

    # ---- quality of a decode ------------------------------------------------------------------------
    @staticmethod
    def convergence_from_sums(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
        """sqrt(num / den) of the two sums of `Plan.spectral_error` (float64).  A silent target (den == 0) gives 0.0 where the
        waveform's spectrum is silent too (num == 0), else inf."""
        ratio = torch.sqrt(num / torch.where(den > 0, den, torch.ones_like(den)))
        silent = torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num))
        return torch.where(den > 0, ratio, silent)

    def spectral_convergence(self, waveform: torch.Tensor, magnitudes: torch.Tensor, loop: bool = False) -> torch.Tensor:
        """
        || |STFT(waveform)| - magnitudes || / || magnitudes || per row, on the device: (B, L) float32 waveforms - L the length
        Griffin-Lim gives T frames, hop * (T - 1) - and (B, n_stft, T) float32 magnitudes in the reference's layout -> (B,) float64.
        The one quality figure of a Griffin-Lim result that does not depend on its random start.  Deterministic: a row's value
        is the same alone and in any batch (rfx_spectral_error).
        `loop`: the waveforms are loop decodes, (B, hop * T), and the STFT is the circular one (rfx_spectral_error_loop).
        """
        plan = self._plan()
        mag = magnitudes.to(self.device)
        B, _, Tn = mag.shape
        sums = plan.spectral_error(waveform.to(self.device), plan.pack_magnitudes(mag), B, Tn, loop=loop)
        return self.convergence_from_sums(sums[:, 0], sums[:, 1])

    # ---- spectral losses for training through the codec ---------------------------------------------
    def spectral_losses(self, waveform: torch.Tensor, magnitudes: T.Optional[torch.Tensor] = None, *,
                        magnitude_slots: T.Optional[torch.Tensor] = None, log_floor: T.Optional[float] = None,
                        loop: bool = False) -> SpectralLosses:
        """
        The pair of the multi-resolution STFT loss at this converter's parameters, fused with the transform on the device:
        `convergence` = || |STFT(waveform)| - M || / || M || and `log_magnitude` = mean | ln max(|STFT(waveform)|, log_floor) -
        ln max(M, log_floor) |, per row: (B, Lw) float32 waveforms -> a named pair of (B,) float64 tensors.  `log_magnitude` is None
        when `log_floor` is None.  The target M is `magnitudes`, (B, n_stft, T) float32 in the reference's layout, or
        `magnitude_slots`, what `plan.pack_magnitudes` returns for it - a training loop packs its constant target once.  It
        receives no gradient: a target that requires grad raises.
        With grad mode on and a waveform that requires grad the pair carries a grad_fn whose backward runs on the device
        (rfx_spectral_loss_backward: the waveform and three sums per row are saved, the spectrum is formed again; the
        (B, n_stft, T) tensor is never written).  Otherwise the forward call alone runs and nothing is saved.  `convergence` is
        `spectral_convergence`'s value bit for bit where that member takes the length.  A multi-resolution loss is the sum of this
        pair over several converters with different parameters.
        `loop`: the rows are whole periods of exactly hop * T samples (`check_loop_samples`) and the STFT is the circular one; this
        is the loop STFT's backward (`mel_amplitudes_from_waveform(loop=True)` has none).
        """
        from riffusion import _hip

        if (magnitudes is None) == (magnitude_slots is None):
            raise ValueError("spectral_losses takes the target once: magnitudes (B, n_stft, T) or magnitude_slots")
        target = magnitudes if magnitudes is not None else magnitude_slots
        if isinstance(target, torch.Tensor) and target.requires_grad:
            raise RuntimeError("spectral_losses: the target receives no gradient; detach it")
        if waveform.dim() != 2:
            raise ValueError(f"spectral_losses takes (B, samples) waveforms, got {tuple(waveform.shape)}")
        f = _hip.spectral_loss_floor(log_floor)
        if log_floor is not None and f == 0.0:
            raise ValueError("log_floor=0 leaves ln 0 in reach; pass None for no log term or a positive floor")
        if loop:
            self.check_loop_samples(int(waveform.shape[-1]))
        plan = self._plan()
        slots = plan.pack_magnitudes(magnitudes.to(self.device)) if magnitudes is not None else magnitude_slots.to(self.device)
        w = waveform.to(self.device)
        sc, lg = _autograd.spectral_losses(plan, w.to(torch.float32) if _autograd.wants_grad(w) else w, slots, f, loop)
        return SpectralLosses(sc, lg if log_floor is not None else None)
