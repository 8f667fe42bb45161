"""
Kernel selection of plan creation, without a GPU.

rfx_plan_create_ex decides on the host which frame engine a geometry runs on, which InverseMelScale kernel a filterbank gets,
whether the gradient's unit form is on and which form the fused forward path takes (csrc/rfx_plan_core.h); the same functions
fill the tables it uploads.  rfx_debug_plan_bank runs them without a device, so the expectations the GPU tests assert through
rfx_plan_imel_kernel / rfx_plan_imel_unit_form / rfx_plan_griffinlim_engine are held here on every machine - on the banks and with
the figures those tests record (named next to each case).
"""
import ctypes

import pytest

from helpers import plan_bank_report


@pytest.fixture(scope="module")
def O():
    import riffusion_oracle

    return riffusion_oracle


def test_default_bank_takes_the_wave_kernel_in_unit_form(O):
    op = O.OracleParams()
    r = plan_bank_report(op)  # tests/test_gpu_full_parity.py
    assert r.imel_ok == 1 and r.imel_why == b"" and (r.imel_kernel, r.unit_form, r.wave_ok, r.fast_ok, r.line_from) == (4, 1, 1, 2, 0)
    assert (r.f_lo, r.f_hi) == (1, 4001) and r.nnz == int((O.mel_filterbank(op) != 0).sum())  # bins 1 .. 4000 (csrc/rfx_kernels.h: kKbMaskLow)
    assert r.engine == 0 and r.frame_stride == 9408


def test_default_bank_without_the_wave_kernel_takes_the_group_kernel(O):
    r = plan_bank_report(O.OracleParams(), imel_form="groups")  # tests/test_gpu_round4.py
    assert (r.imel_kernel, r.wave_ok, r.unit_form) == (2, 0, 1)


def test_normalised_htk_bank_takes_the_wave_kernel_without_the_unit_form(O):
    r = plan_bank_report(O.OracleParams(mel_scale_type="htk", mel_scale_norm="slaney"))  # tests/test_gpu_round3_parity.py
    assert (r.imel_kernel, r.unit_form) == (4, 0)


# tests/test_gpu_round5.py::test_line_form_group_kernel_on_banks_with_long_groups
LINE_FORM_BANKS = [(dict(min_frequency=20, max_frequency=20000), 1), (dict(max_frequency=22050), 1), (dict(max_frequency=16000, mel_scale_norm="slaney"), 0),
                   (dict(max_frequency=20000, mel_scale_type="slaney"), 1), (dict(num_frequencies=384), 1), (dict(num_frequencies=256), 0),
                   (dict(num_frequencies=300, max_frequency=12000), 1), (dict(num_frequencies=200), 0), (dict(sample_rate=48000, max_frequency=20000), 1)]


@pytest.mark.parametrize("kw,unit", LINE_FORM_BANKS)
def test_banks_with_long_groups_take_the_line_form_group_kernel(O, kw, unit):
    r = plan_bank_report(O.OracleParams(**kw))
    assert (r.imel_kernel, r.fast_ok, r.unit_form, r.wave_ok) == (5, 5, unit, 0)


def test_a_step_count_that_outgrows_64_kb_of_lds_takes_the_general_kernel(O):
    kw = dict(min_frequency=20, max_frequency=20000)  # tests/test_gpu_round6.py
    assert plan_bank_report(O.OracleParams(max_mel_iters=2000, **kw)).imel_kernel == 0
    assert plan_bank_report(O.OracleParams(max_mel_iters=200, **kw)).imel_kernel == 5


@pytest.mark.parametrize("kw,opt,engine", [(dict(), {}, 0), (dict(sample_rate=48000), {}, 2), (dict(sample_rate=48000), dict(frame_engine="generic"), 1),
                                           (dict(sample_rate=11025, max_frequency=5000), {}, 1), (dict(sample_rate=96000), {}, 1)])
def test_frame_engine_by_geometry(O, kw, opt, engine):
    op = O.OracleParams(**kw)
    r = plan_bank_report(op, **opt)
    assert r.engine == engine
    assert r.frame_stride == (9408 if engine == 0 else (op.n_stft + 63) // 64 * 64)  # slot-major, or plain bin-ordered frames
    assert plan_bank_report(op, fb=None, **opt).engine == engine  # the geometry decides, with or without a bank


def test_unsupported_fft_length_is_refused_with_a_reason(O):
    from riffusion import _hip

    p = O.OracleParams(sample_rate=42570)  # tests/test_gpu_generic_geometry.py: n_fft = 17028 = 2^2 * 3^2 * 11 * 43
    assert p.n_fft == 17028
    with pytest.raises(_hip.RfxError, match="prime factor above 13"):
        plan_bank_report(p)
    with pytest.raises(_hip.RfxError, match="does not fit the 160 KiB of LDS"):
        plan_bank_report(O.OracleParams(sample_rate=192000, max_frequency=10000))  # n_fft 76800: 38400 complex numbers = 300 KiB


# tests/test_gpu_round5.py::FWD_CASES: (fwd_ok, product form, packed tables)
@pytest.mark.parametrize("kw,forms", [(dict(), (1, 1, 1)), (dict(min_frequency=20, max_frequency=20000), (1, 1, 0)),
                                      (dict(num_frequencies=700, max_frequency=10000), (1, 0, 0)),
                                      (dict(sample_rate=48000, max_frequency=10000), (1, 0, 0)), (dict(sample_rate=11025, max_frequency=5000), (1, 0, 0))])
def test_forward_path_form_by_bank(O, kw, forms):
    op = O.OracleParams(**kw)
    r = plan_bank_report(op)
    assert (r.fwd_ok, r.fwd_product, r.fwd_packed) == forms
    assert r.Mpad == (op.num_frequencies + 63) // 64 * 64 and r.band_rows % 8 == 0 and r.band_rows > 0
    if forms[2]:  # csrc/rfx_kernels.h: kKbMaskLow, kMelProdArr - the compile-time set and distance of the packed kernel
        assert r.fwd_kb_mask == 0x1F001F and r.fwd_prod_arr == 8192
    elif forms[1]:
        assert r.fwd_kb_mask & ~0x1F001F and r.fwd_kb_mask <= 0x1FFFFF and r.fwd_prod_arr > 0
    else:
        assert r.fwd_kb_mask == 0 and r.fwd_prod_arr == 0


def test_a_bank_that_is_not_banded_is_reported_with_its_reason(O):
    import torch

    op = O.OracleParams(num_frequencies=16)
    fb = torch.rand(op.n_stft, 16, generator=torch.Generator().manual_seed(0))
    r = plan_bank_report(op, fb=fb)
    assert r.imel_ok == 0 and r.imel_kernel == -1 and r.fwd_ok == 0 and b"more than two adjacent mel filters" in r.imel_why
    r = plan_bank_report(op, fb=None)
    assert r.imel_ok == 0 and r.imel_kernel == -1 and r.engine == 0


def test_report_is_struct_size_led(O):
    """A caller built against a shorter report gets the fields it knows and not a byte more."""
    from riffusion import _hip

    op = O.OracleParams()
    fb = O.mel_filterbank(op).contiguous()
    cp = _hip.RfxParams(op.sample_rate, op.n_fft, op.win_length, op.hop_length, op.num_frequencies, op.max_mel_iters)
    lib = _hip.load_library()
    buf = (ctypes.c_ubyte * ctypes.sizeof(_hip.RfxPlanBankReport))(*([0xAB] * ctypes.sizeof(_hip.RfxPlanBankReport)))
    rep = _hip.RfxPlanBankReport.from_buffer(buf)
    rep.struct_size = 20
    assert lib.rfx_debug_plan_bank(ctypes.byref(cp), fb.data_ptr(), None, ctypes.byref(rep)) == 0
    assert (rep.struct_size, rep.engine, rep.frame_stride, rep.imel_ok, rep.imel_kernel) == (20, 0, 9408, 1, 4) and all(b == 0xAB for b in buf[20:])
    for bad in (4, ctypes.sizeof(_hip.RfxPlanBankReport) + 4):
        rep.struct_size = bad
        assert lib.rfx_debug_plan_bank(ctypes.byref(cp), fb.data_ptr(), None, ctypes.byref(rep)) == -1
        assert b"struct_size" in lib.rfx_last_error()
