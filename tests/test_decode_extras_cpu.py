"""The two values the Python layers hand a decode call's extras down in (riffusion/_decode.py): how `ClipExtras.rows` lowers a
chunk of clips to the rows of one library call, that the options struct made of a lowered value is the one the loose keywords
make, and that every layer still refuses what it refused, in its own words and in the same order.  CPU tensors, no device."""
import numpy as np
import pytest
import torch

N, W, M = 5, 48, 16
CHUNKS = ((0, 2), (2, 4), (4, 5))


class _Lib:
    """stands in for librfx.so where a plan only asks it for sizes"""

    def __getattr__(self, name):
        return lambda *a: 2 if name == "rfx_hold_mask_words" else 0


def _plan():
    """a Plan without a handle: its checks and its option building run, nothing else"""
    from riffusion import _hip

    plan = _hip.Plan.__new__(_hip.Plan)
    plan.lib, plan.handle, plan.device = _Lib(), None, torch.device("cpu")
    plan.hop_length, plan.n_fft, plan.n_stft, plan.n_mels, plan.frame_stride, plan.griffinlim_engine = 441, 17640, 8821, M, 64, "fft"
    plan.lstsq_ok, plan.seen = True, []

    def hold_bins_from_bands(bands):  # any function of a row's bands alone: two bands' bits per frame, (B, T, 2) int32
        plan.seen.append(bands)
        return torch.stack([bands[:, 0, :].to(torch.int32), bands[:, M - 1, :].to(torch.int32) << 3], dim=2).contiguous()

    plan.hold_bins_from_bands = hold_bins_from_bands
    return plan


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("guide_channels", ["C", 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_rows_lowers_a_chunk_by_the_batch_entrys_formulas(C, guide_channels, dtype):
    from riffusion._decode import ClipExtras, DecodeExtras
    from riffusion.spectrogram_converter import hold_rows

    gen = torch.Generator().manual_seed(7)
    guides = (torch.rand((N, C if guide_channels == "C" else 1, 37), generator=gen) * 2000 - 1000).to(dtype)
    holds = hold_rows((3, 2), N, W)
    bands = (torch.rand((N, M, W), generator=gen) < 0.5).to(torch.uint8)
    plan, dev = _plan(), torch.device("cpu")
    clips = ClipExtras(guides=guides, holds=holds, bands=bands, loop=True, peak_start=True, inverse_mel="lstsq", n_iter=2)
    for a, b in CHUNKS:
        want_guide = guides[a:b].to(dev, torch.float32).expand(b - a, C, 37).reshape((b - a) * C, 37)
        want_hold = holds[a:b].to(dev).repeat_interleave(C, 0).contiguous()
        want_bands = bands[a:b].to(dev).repeat_interleave(C, 0).contiguous()
        staged = clips.rows(plan, (a, b, C))
        assert torch.equal(plan.seen[-1], want_bands) and plan.seen[-1].is_contiguous()  # the staged calls expand the rows' bands
        fused = clips.rows(plan, (a, b, C), bins_first=True)
        assert torch.equal(plan.seen[-1], bands[a:b])  # the fused call expands the clips' bands and gives the bins to the rows
        want_bins = plan.hold_bins_from_bands(bands[a:b].to(dev)).repeat_interleave(C, 0).contiguous()
        for x in (staged, fused):
            assert isinstance(x, DecodeExtras) and (x.loop, x.peak_start, x.lstsq) == (True, True, True)
            assert x.guide.dtype == torch.float32 and torch.equal(x.guide, want_guide)
            assert x.hold.dtype == torch.int32 and torch.equal(x.hold, want_hold) and x.hold.is_contiguous()
            assert torch.equal(x.hold_bins, want_bins) and x.hold_bins.is_contiguous()
    # an absent member lowers to None, and the plain decode to the plain call
    for a, b in CHUNKS:
        assert ClipExtras().rows(plan, (a, b, C)) == DecodeExtras()
        only_guides = ClipExtras(guides=guides).rows(plan, (a, b, C), bins_first=True)
        assert (only_guides.hold, only_guides.hold_bins, only_guides.loop, only_guides.peak_start, only_guides.lstsq) == (None, None, False, False, False)
        assert ClipExtras(holds=holds).rows(plan, (a, b, C)).guide is None
    # every flag lowers to its own member
    assert ClipExtras(loop=True).rows(plan) == DecodeExtras(loop=True) and ClipExtras(peak_start=True).rows(plan, (0, 2, C)) == DecodeExtras(peak_start=True)
    assert ClipExtras(inverse_mel="lstsq", n_iter=3).rows(plan) == DecodeExtras(lstsq=True)
    # entries that are rows already (`waveform_from_mel_amplitudes`): moved to the device, nothing sliced or repeated
    rows = ClipExtras(guides=guides[:, 0], holds=holds, bands=bands).rows(plan)
    assert torch.equal(rows.guide, guides[:, 0].to(torch.float32)) and torch.equal(rows.hold, holds) and torch.equal(plan.seen[-1], bands)


def _variants(R, T):
    g = torch.zeros((R, 50))
    h = torch.ones((R, 2), dtype=torch.int32)
    m = torch.zeros((R, T, 2), dtype=torch.int32)
    return {"none": {}, "guide": dict(guide=g), "guide + hold": dict(guide=g, hold=h), "guide + bins": dict(guide=g, hold_bins=m), "loop": dict(loop=True),
            "loop + guide": dict(loop=True, guide=g), "peaks": dict(peak_start=True), "lstsq alone": dict(lstsq=True)}


@pytest.mark.parametrize("name", list(_variants(1, 1)))
def test_a_lowered_value_makes_the_struct_the_loose_keywords_make(name):
    """through `Plan._inverse_call`, as the three public entries build their options"""
    from riffusion import _hip
    from riffusion._decode import DecodeExtras

    R, T = 4, 41
    kw = _variants(R, T)[name]
    loose = _hip.call_options(rows=R, row_base=6, magnitude_hint=2.5, **kw)
    opt, need, _ = _plan()._inverse_call("waveform_from_mel", (R, T), R, T, 6, 2.5, DecodeExtras(**kw))
    assert type(opt) is type(loose) and bytes(opt) == bytes(loose) and need == 0
    assert type(opt) is {"none": _hip.RfxCallOptions, "guide": _hip.RfxGuidedCallOptions, "guide + hold": _hip.RfxHeldCallOptions,
                         "guide + bins": _hip.RfxMaskedCallOptions, "loop": _hip.RfxLoopCallOptions, "loop + guide": _hip.RfxLoopCallOptions,
                         "peaks": _hip.RfxStartCallOptions, "lstsq alone": _hip.RfxCallOptions}[name]
    assert DecodeExtras.fold(None, **kw) == DecodeExtras(**kw) and DecodeExtras.fold(DecodeExtras(**kw)) == DecodeExtras(**kw)
    if kw:
        with pytest.raises(TypeError, match="not both"):
            DecodeExtras.fold(DecodeExtras(), **kw)


# ---- refusals ----------------------------------------------------------------------------------------------------------
_R, _T = 3, 41


def _t():
    """the tensors the cases name"""
    return dict(g=torch.zeros((_R, 50)), h=torch.ones((_R, 2), dtype=torch.int32), m=torch.zeros((_R, _T, 2), dtype=torch.int32),
                a0=torch.zeros((_R * _T, 64), dtype=torch.complex64), mag=torch.zeros((_R * _T, 64)), mel=torch.zeros((_R, M, _T)),
                mel1=torch.zeros((1, 512, 40)), g1=torch.zeros((1, 1000)), a1=torch.zeros((1, 8821, 40), dtype=torch.complex64),
                bands1=np.zeros((1, 512, 40), bool), tiles=np.zeros((1, M, 40, 3), np.uint8), guides=np.zeros((1, 1, 100), np.float32),
                bands=np.zeros((1, M, 40), bool), img=torch.zeros((1, M, _T, 3), dtype=torch.uint8), lut=torch.zeros(256))


def _call(entry, kw):
    """one public entry on the arguments `kw` names (strings are looked up in `_t`)"""
    from riffusion import _hip, cli
    from riffusion.spectrogram_converter import SpectrogramConverter
    from riffusion.spectrogram_image_converter import SpectrogramImageConverter
    from riffusion.spectrogram_params import SpectrogramParams

    t = _t()
    kw = {k: t[v] if isinstance(v, str) and v in t else v for k, v in kw.items()}
    if entry == "call_options":
        return _hip.call_options(rows=_R, **kw)
    if entry == "check_phase_start":
        return _hip.check_phase_start("peaks", **kw)
    if entry == "cli.image_to_audio":
        return cli.image_to_audio(image="x.png", audio="y.wav", **kw)
    if entry.startswith("Plan."):
        if entry.endswith("[extras]"):
            from riffusion._decode import DecodeExtras

            kw = dict({k: kw.pop(k) for k in list(kw) if k == "angles0_slots"}, extras=DecodeExtras(**kw))
        if entry.startswith("Plan.griffinlim"):
            return _plan().griffinlim(t["mag"], _R, _T, 2, **kw)
        if entry.startswith("Plan.waveform_from_mel"):
            return _plan().waveform_from_mel(t["mel"], 1, 2, **kw)
        return _plan().audio_from_image(t["img"], False, t["lut"], 2, **{k: v[:1] if torch.is_tensor(v) else v for k, v in kw.items()})
    if entry == "waveform_from_mel_amplitudes":
        return SpectrogramConverter.__new__(SpectrogramConverter).waveform_from_mel_amplitudes(t["mel1"], **kw)
    ic = SpectrogramImageConverter.__new__(SpectrogramImageConverter)
    ic.p = SpectrogramParams(num_frequencies=M)
    ic.converter = type("Conv", (), {"_plan": staticmethod(_plan), "p": ic.p})()
    if entry == "audio_from_spectrogram_image":
        return ic.audio_from_spectrogram_image(None, **kw)
    return getattr(ic, entry)(t["tiles"], **kw)


PEAKS = dict(phase_start="peaks")
REFUSALS = [  # (entry, its arguments, the rules they break, the parent commit's message)
    # BUILDER_WORDING
    ("call_options", dict(peak_start=True, guide="g"), "peak_start",
     "peak_start together with guide, hold or hold_bins is not served: each is a start, or needs the guide's"),
    ("call_options", dict(loop=True, guide="g", hold="h"), "loop_holds", "loop together with hold or hold_bins is not served"),
    ("call_options", dict(hold="h"), "hold_needs_guide", "hold needs a guide: the frames are held at the guide's phase"),
    ("call_options", dict(hold_bins="m"), "bins_need_guide", "hold_bins needs a guide: the bins are held at the guide's phase"),
    ("call_options", dict(guide="g", hold="h", hold_bins="m"), "bins_and_hold",
     "hold_bins together with hold is not served: set the held frames' bits in the mask"),
    ("call_options", dict(peak_start=True, loop=True, guide="g", hold="h"), "peak_start + loop_holds",
     "peak_start together with guide, hold or hold_bins is not served: each is a start, or needs the guide's"),
    ("call_options", dict(hold="h", hold_bins="m"), "hold_needs_guide + bins_need_guide + bins_and_hold",
     "hold needs a guide: the frames are held at the guide's phase"),
    # PLAN_WORDING
    ("Plan.griffinlim", dict(loop=True, guide="g", hold="h"), "loop_holds", "loop together with hold or hold_bins is not served"),
    ("Plan.griffinlim", dict(peak_start=True, guide="g"), "peak_start",
     "peak_start does not go with guide: the peak start needs no guide and holds nothing"),
    ("Plan.griffinlim", dict(peak_start=True, angles0_slots="a0"), "peak_start",
     "peak_start does not go with angles0_slots: the peak start needs no guide and holds nothing"),
    ("Plan.griffinlim", dict(guide="g", angles0_slots="a0"), "two_starts", "a guide and angles0_slots are two starts: give one"),
    ("Plan.griffinlim", dict(hold="h"), "hold_needs_guide", "hold needs a guide: the frames are held at the guide's phase"),
    ("Plan.griffinlim", dict(hold_bins="m"), "bins_need_guide", "hold_bins needs a guide: the bins are held at the guide's phase"),
    ("Plan.griffinlim", dict(guide="g", hold="h", hold_bins="m"), "bins_and_hold",
     "hold_bins together with hold is not served: set the held frames' bits in the mask"),
    ("Plan.griffinlim", dict(loop=True, peak_start=True, guide="g", hold="h"), "loop_holds + peak_start",
     "loop together with hold or hold_bins is not served"),
    ("Plan.griffinlim", dict(peak_start=True, guide="g", angles0_slots="a0", hold_bins="m"), "peak_start + two_starts",
     "peak_start does not go with angles0_slots, guide, hold_bins: the peak start needs no guide and holds nothing"),
    ("Plan.waveform_from_mel", dict(peak_start=True, guide="g", hold="h"), "peak_start",
     "peak_start does not go with guide, hold: the peak start needs no guide and holds nothing"),
    ("Plan.waveform_from_mel", dict(hold="h", hold_bins="m"), "hold_needs_guide + bins_need_guide + bins_and_hold",
     "hold needs a guide: the frames are held at the guide's phase"),
    ("Plan.audio_from_image", dict(loop=True, guide="g", hold_bins="m"), "loop_holds", "loop together with hold or hold_bins is not served"),
    ("Plan.audio_from_image", dict(lstsq=True, hold_bins="m"), "bins_need_guide", "hold_bins needs a guide: the bins are held at the guide's phase"),
    # CALL_WORDING
    ("waveform_from_mel_amplitudes", dict(PEAKS, guide="g1"), "peak_start",
     'phase_start="peaks" does not go with guide: the peak start needs no guide and holds nothing'),
    ("waveform_from_mel_amplitudes", dict(loop=True, guide="g1", hold_frames=(1, 1)), "loop_holds",
     "loop together with hold_frames or hold_mask is not served"),
    ("waveform_from_mel_amplitudes", dict(guide="g1", angles0="a1"), "two_starts", "guide and angles0 are two starts of Griffin-Lim: give one"),
    ("waveform_from_mel_amplitudes", dict(hold_frames=(1, 1)), "hold_needs_guide",
     "hold_frames needs a guide: the frames are held at the guide's phase"),
    ("waveform_from_mel_amplitudes", dict(hold_mask="bands1"), "bins_need_guide", "hold_mask needs a guide: the bins are held at the guide's phase"),
    ("waveform_from_mel_amplitudes", dict(guide="g1", hold_frames=(1, 1), hold_mask="bands1"), "bins_and_hold",
     "hold_frames together with hold_mask is not served: set the held frames' columns in the mask"),
    ("waveform_from_mel_amplitudes", dict(PEAKS, loop=True, guide="g1", hold_frames=(1, 1)), "peak_start + loop_holds",
     'phase_start="peaks" does not go with guide, hold_frames: the peak start needs no guide and holds nothing'),
    ("waveform_from_mel_amplitudes", dict(loop=True, guide="g1", angles0="a1", hold_mask="bands1"), "loop_holds + two_starts",
     "loop together with hold_frames or hold_mask is not served"),
    ("waveform_from_mel_amplitudes", dict(hold_frames=(1, 1), hold_mask="bands1"), "hold_needs_guide + bins_need_guide + bins_and_hold",
     "hold_frames needs a guide: the frames are held at the guide's phase"),
    ("audio_from_spectrogram_image", dict(PEAKS, guide_segment=object()), "peak_start",
     'phase_start="peaks" does not go with guide_segment: the peak start needs no guide and holds nothing'),
    ("audio_from_spectrogram_image", dict(hold_frames=(1, 1), hold_mask="bands"), "hold_needs_guide + bins_need_guide",
     "hold_frames needs a guide: the frames are held at the guide's phase"),
    ("audio_from_spectrogram_image", dict(hold_mask="bands"), "bins_need_guide", "hold_mask needs a guide: the bins are held at the guide's phase"),
    # BATCH_WORDING
    ("audio_from_spectrogram_images", dict(PEAKS, guide_waveforms="guides"), "peak_start",
     'phase_start="peaks" does not go with guide_waveforms: the peak start needs no guide and holds nothing'),
    ("audio_from_spectrogram_images", dict(loop=True, guide_waveforms="guides", hold_frames=(1, 1)), "loop_holds",
     "loop together with hold_frames or hold_mask is not served"),
    ("audio_from_spectrogram_images", dict(hold_frames=(1, 1)), "hold_needs_guide",
     "hold_frames needs guide_waveforms: the frames are held at the guides' phase"),
    ("audio_from_spectrogram_images", dict(hold_mask="bands"), "bins_need_guide", "hold_mask needs guide_waveforms: the bins are held at the guides' phase"),
    ("audio_from_spectrogram_images", dict(guide_waveforms="guides", hold_frames=(1, 1), hold_mask="bands"), "bins_and_hold",
     "hold_frames together with hold_mask is not served: set the held frames' columns in the mask"),
    ("audio_from_spectrogram_images", dict(PEAKS, loop=True, guide_waveforms="guides", hold_mask="bands"), "peak_start + loop_holds",
     'phase_start="peaks" does not go with guide_waveforms, hold_mask: the peak start needs no guide and holds nothing'),
    ("audio_from_spectrogram_images", dict(hold_frames=(1, 1), hold_mask="bands"), "hold_needs_guide + bins_need_guide + bins_and_hold",
     "hold_frames needs guide_waveforms: the frames are held at the guides' phase"),
    ("audio_from_spectrogram_images", dict(loop=True, hold_frames=(1, 1), return_error=True), "loop_holds, before the entry's own loop refusal",
     "loop together with hold_frames or hold_mask is not served"),
    ("audio_from_spectrogram_image_sequence", dict(PEAKS, guide_waveforms="guides"), "peak_start",
     'phase_start="peaks" does not go with guide_waveforms: the peak start needs no guide and holds nothing'),
    ("audio_from_spectrogram_image_sequence", dict(hold_mask="bands"), "bins_need_guide",
     "hold_mask needs guide_waveforms: the bins are held at the guides' phase"),
    ("audio_from_spectrogram_image_sequence", dict(PEAKS, hold_mask="bands"), "peak_start + bins_need_guide",
     'phase_start="peaks" does not go with hold_mask: the peak start needs no guide and holds nothing'),
    # PEAKS_WORDING and the command line's flags
    ("check_phase_start", dict(angles0="a1", guide="g1"), "peak_start",
     'phase_start="peaks" does not go with angles0, guide: the peak start needs no guide and holds nothing'),
    ("cli.image_to_audio", dict(PEAKS, guide_audio="g.wav"), "peak_and_guide", "--phase-start peaks does not go with --guide-audio: they are two starts"),
    ("cli.image_to_audio", dict(loop=True, hold_mask="m.png", hold_head_ms=5), "loop_holds + bins_need_guide + bins_and_hold + hold_needs_guide",
     "--loop does not go with --hold-head-ms / --hold-tail-ms / --hold-mask"),
    ("cli.image_to_audio", dict(hold_mask="m.png", hold_head_ms=5), "bins_need_guide + bins_and_hold + hold_needs_guide",
     "--hold-mask needs --guide-audio: the bins are held at the guide's phase"),
]


@pytest.mark.parametrize("entry,kw,rules,message", REFUSALS, ids=[f"{i:02d}-{r[0]}-{r[2].replace(' ', '')}" for i, r in enumerate(REFUSALS)])
def test_every_layer_refuses_in_its_words_and_order(entry, kw, rules, message):
    """The messages are the parent commit's: its `riffusion` package was exported beside the tree
    (`git archive <parent> riffusion-hobby_amd/riffusion | tar -x -C <dir>`), put first on sys.path with RFX_LIB_PATH naming the
    built library, and `_call(entry, kw)` of this module run on every row of the table; the ValueError's text is the row's last
    column.  A plan entry refuses the same whether its extras come as keywords or as a ready `DecodeExtras`."""
    with pytest.raises(ValueError) as e:
        _call(entry, dict(kw))
    assert str(e.value) == message
    if entry.startswith("Plan."):
        with pytest.raises(ValueError) as e:
            _call(entry + "[extras]", dict(kw))
        assert str(e.value) == message


def test_the_table_covers_every_rule_and_two_at_once_in_every_wording():
    single = {rules for _, _, rules, _ in REFUSALS if " " not in rules}
    assert single == {"peak_start", "peak_and_guide", "loop_holds", "two_starts", "hold_needs_guide", "bins_need_guide", "bins_and_hold"}
    for layer in ("call_options", "Plan.", "waveform_from_mel_amplitudes", "audio_from_spectrogram_images", "cli."):
        assert any(entry.startswith(layer) and "+" in rules for entry, _, rules, _ in REFUSALS), layer
