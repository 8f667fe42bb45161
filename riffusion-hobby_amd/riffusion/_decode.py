"""
What a decode call has beyond magnitudes and a seed, as two values the Python layers hand down whole:

    DecodeExtras  the extras of ONE library call, row for row: what `_hip.call_options` makes a struct of
    ClipExtras    the extras of a converter call, clip for clip, on any device; `rows` lowers tiles [a, b) to a DecodeExtras

Neither checks a combination rule: `_hip.check_call_rules` states the rules, and every layer calls it in its own words where it
takes the arguments from its caller.
"""
import dataclasses
import typing as T

import torch


@dataclasses.dataclass(frozen=True)
class DecodeExtras:
    """`guide` (rows, Lg) float32, `hold` (rows, 2) int32, `hold_bins` (rows, T, words) int32, `loop`, `peak_start` and `lstsq` as
    `_hip.call_options` documents them."""

    guide: T.Optional[torch.Tensor] = None
    hold: T.Optional[torch.Tensor] = None
    hold_bins: T.Optional[torch.Tensor] = None
    loop: bool = False
    peak_start: bool = False
    lstsq: bool = False

    @classmethod
    def fold(cls, extras: T.Optional["DecodeExtras"], **loose: T.Any) -> "DecodeExtras":
        """What a public door does with its keywords: the ready value if the caller brought one (then no loose keyword beside
        it), otherwise the value of the keywords."""
        if extras is None:
            return cls(**loose)
        if any(value is not None and value is not False for value in loose.values()):
            raise TypeError("give the decode extras as `extras` or as keywords, not both")
        return extras

    def starts_and_holds(self) -> T.Dict[str, T.Any]:
        """the members the combination rules are about, as `_hip.check_call_rules` takes them"""
        return dict(guide=self.guide, hold=self.hold, hold_bins=self.hold_bins, loop=self.loop, peak_start=self.peak_start)


@dataclasses.dataclass(frozen=True)
class ClipExtras:
    """A converter call's extras, one entry per clip: `guides` (N, C or 1, Lg) float32 or int16, `holds` (N, 2) int32
    (`hold_rows`), `bands` (N, n_mels, W) uint8 (`hold_mask_rows`), each on any device or None; the flags; `n_iter`: Griffin-Lim's
    iterations (None: the params').  The default is the plain decode."""

    guides: T.Optional[torch.Tensor] = None
    holds: T.Optional[torch.Tensor] = None
    bands: T.Optional[torch.Tensor] = None
    loop: bool = False
    peak_start: bool = False
    inverse_mel: str = "sgd"
    n_iter: T.Optional[int] = None

    def rows(self, plan: T.Any, tiles: T.Optional[T.Tuple[int, int, int]] = None, bins_first: bool = False) -> DecodeExtras:
        """The extras of one library call on the plan's device.  `tiles=(a, b, C)`: the call decodes clips [a, b) with C channel
        rows each, and every row gets its clip's entry (a mono guide serves both rows of a stereo tile); None: the entries are
        the call's rows already ((B, Lg) guides).  `bins_first`: the bands are expanded to bins clip by clip and then given to
        the rows (the fused call); otherwise row by row (the staged calls)."""
        a, b, C = tiles if tiles is not None else (None, None, 1)

        def on_device(t: torch.Tensor, *dtype: torch.dtype) -> torch.Tensor:
            return (t if tiles is None else t[a:b]).to(plan.device, *dtype)

        def per_row(t: torch.Tensor) -> torch.Tensor:
            return t if tiles is None else t.repeat_interleave(C, dim=0).contiguous()

        guide = hold = hold_bins = None
        if self.guides is not None:
            guide = on_device(self.guides, torch.float32)
            if tiles is not None:
                guide = guide.expand(b - a, C, guide.shape[2]).reshape((b - a) * C, guide.shape[2])
        if self.holds is not None:
            hold = per_row(on_device(self.holds))
        if self.bands is not None:
            bands = on_device(self.bands)
            hold_bins = per_row(plan.hold_bins_from_bands(bands)) if bins_first else plan.hold_bins_from_bands(per_row(bands))
        return DecodeExtras(guide, hold, hold_bins, self.loop, self.peak_start, self.inverse_mel == "lstsq")
