"""
Griffin-Lim run form with one audio buffer per generation except at run seams (rfx_gl.hip): buffer 1 of a generation holds only
what a run adds to the nine hop blocks it shares with the previous run of its row, a group boundary INSIDE a run is merged by the
thread that owns both partial sums, and every reader - the next launch, the launch after it, gl_combine_kernel - adds buffer 1
only in those nine blocks.  The per-frame form (gl_frame_kernel + gl_fold_kernel) knows nothing of runs or buffers: every case
here asks both forms for the same call and wants the same float waveform.

Shapes: T = 33 is groups of 16, 16 and 1 frames (a boundary five blocks from the row's end: the reflect padding reads its nine
blocks), T = 48 three whole groups.  With few rows every group is a run of its own (seams between runs only); the two large
batches are sized from the device's own partition so that runs hold 1 and 2, and 2 and 3 groups - a seam inside a run - and
cross from one row into the next.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GROUP = 16
ITERS = (0, 1, 4)


def _plans():
    from riffusion import _hip
    from riffusion.spectrogram_params import SpectrogramParams

    p = SpectrogramParams()
    return _hip.get_plan(p, "cuda", gl_form="runs"), _hip.get_plan(p, "cuda", gl_form="frames")


def _run_starts(plan, B, Tn):
    cap = 1 << 16
    starts = (ctypes.c_int64 * cap)()
    n = plan.lib.rfx_griffinlim_runs(plan.handle, B, Tn, 0, ctypes.cast(starts, ctypes.c_void_p), cap)
    assert 0 < n < cap
    return list(starts[: n + 1])


def _slots(plan):
    """resident workgroup slots of the device: the number of runs of a batch with more groups than that"""
    return len(_run_starts(plan, 20000, 33)) - 1


def _seams(starts, Tn):
    """(group counts of the runs, a run crosses a row, a run holds a group boundary inside a row, two runs meet inside a row)"""
    ng = (Tn + GROUP - 1) // GROUP
    unit = lambda f: (f // Tn) * ng + (f % Tn) // GROUP  # noqa: E731
    sizes, crosses, inner, outer = set(), False, False, False
    for a, b in zip(starts, starts[1:]):
        ua, ub = unit(a), unit(b - 1)
        sizes.add(ub - ua + 1)
        crosses |= a // Tn != (b - 1) // Tn
        inner |= any(u % ng != 0 for u in range(ua + 1, ub + 1))
        outer |= a % Tn != 0
    return sizes, crosses, inner, outer


def _magnitudes(plan, B, Tn, seed, zero_row=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    S = torch.rand(B * Tn, plan.frame_stride, device="cuda", generator=g) * 1000.0
    if zero_row is not None:
        S[zero_row * Tn:(zero_row + 1) * Tn] = 0.0
    return plan.pack_magnitudes(plan.unpack_magnitudes(S, B, Tn))  # a bin held in two slots: the same value in both


def _same(runs, frames, S, B, Tn, iters=ITERS, **kw):
    for n_iter in iters:
        a = runs.griffinlim(S, B, Tn, n_iter, 0.99, seed=31, row_base=11, **kw)
        b = frames.griffinlim(S, B, Tn, n_iter, 0.99, seed=31, row_base=11, **kw)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, b), f"B={B} T={Tn} n_iter={n_iter}: {int((a != b).sum())} of {a.numel()} samples differ"


@pytest.mark.parametrize("Tn", [33, 48])
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_every_group_its_own_run(B, Tn):
    """Few rows: one run per group, so every group boundary of a row is a seam between two workgroups (buffer 1 written by one,
    buffer 0 by the other) and every row boundary a run boundary that shares nothing."""
    runs, frames = _plans()
    starts = _run_starts(runs, B, Tn)
    sizes, crosses, inner, outer = _seams(starts, Tn)
    assert sizes == {1} and not crosses and not inner and outer
    n = runs.lib.rfx_debug_gl_partition(_slots(runs), B, Tn, None, 0)
    assert n == len(starts) - 1
    _same(runs, frames, _magnitudes(runs, B, Tn, 9 * B + Tn), B, Tn)


@pytest.mark.parametrize("which", ["1_and_2_groups", "2_and_3_groups"])
def test_runs_of_several_groups_across_rows(which):
    """More groups than workgroup slots (T = 33: three groups per row): runs of 1 and 2, or of 2 and 3 groups.  A run then holds
    a group boundary (merged in registers through L2), crosses from one row into the next (nothing shared) and still meets its
    neighbour inside a row (two buffers)."""
    runs, frames = _plans()
    Tn, slots = 33, _slots(runs)
    B = slots // 3 + 2 if which == "1_and_2_groups" else (2 * slots) // 3 + 2
    sizes, crosses, inner, outer = _seams(_run_starts(runs, B, Tn), Tn)
    assert sizes == ({1, 2} if which == "1_and_2_groups" else {2, 3}) and crosses and inner and outer
    S = _magnitudes(runs, B, Tn, 7)
    _same(runs, frames, S, B, Tn)
    L = 441 * (Tn - 1)
    guide = torch.randn(B, L, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.1
    _same(runs, frames, S, B, Tn, iters=(4,), guide=guide)


def test_guided_start_reads_the_staged_guide_through_one_buffer():
    """A guided call's launch 0 analyses the staged guide (buffer 0 the guide, buffer 1 zeros) by the same reader rule."""
    runs, frames = _plans()
    B, Tn = 5, 33
    guide = torch.randn(B, 441 * (Tn - 1) + 100, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    _same(runs, frames, _magnitudes(runs, B, Tn, 21), B, Tn, guide=guide)


def test_an_all_zero_tile_keeps_its_zeros():
    """A row of zero magnitudes between two ordinary ones: every sample of it is zero in both forms (a block that gets no second
    addend is still lo s + hi s with lo = 0, never a bare product), and its neighbours are untouched by it."""
    runs, frames = _plans()
    B, Tn = 3, 33
    S = _magnitudes(runs, B, Tn, 5, zero_row=1)
    _same(runs, frames, S, B, Tn)
    a = runs.griffinlim(S, B, Tn, 4, 0.99, seed=31, row_base=11)
    b = frames.griffinlim(S, B, Tn, 4, 0.99, seed=31, row_base=11)
    assert not bool(a[1].any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
