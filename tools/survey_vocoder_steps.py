"""
Time stretch: at which rates does torch's own arange pick another frame pair than the stated step positions?

    python tools/survey_vocoder_steps.py [--frames 512] [--out profiles/time_stretch_steps.txt]     (host only, no GPU)

include/rfx.h ("TIME STRETCH") and tests/vocoder_oracle.py put output step i at the double product x = (double)i * rate and take the
frame pair (floor(x), floor(x) + 1).  torchaudio.functional.phase_vocoder takes its steps from torch.arange(0, T, rate) in the
spectrogram's real dtype, and arange's value for step i is not that product: where i * rate lies within rounding of an integer the
two can fall on different sides of it, and the step interpolates the neighbouring pair - the same magnitude to rounding (the weight
is then next to 0 or 1), another phase increment, and from that step on another accumulated phase.

The survey: every reduced fraction p/q in [0.25, 4] with q <= 24 and p <= 48 - what `--bpm-from A --bpm-to B` produces - at T = `--frames`
frames.  Per rate it counts the steps whose floor differs between the double product and (a) the float64 CPU arange, (b) the float32
CPU arange (what torchaudio forms for a float32 spectrogram).  It prints the totals, the rates with the most differing steps, and
the first differing step of a few familiar ratios.  Recorded, not gated: the figures describe the torch build that ran the tool.
"""
import argparse
import math
import os
import sys
from fractions import Fraction

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIAR = [(2, 3), (4, 3), (3, 10), (6, 5), (5, 6), (3, 2), (5, 4), (3, 4), (11, 10), (9, 10), (2, 1), (3, 1)]


def fractions():
    return sorted({Fraction(p, q) for q in range(1, 25) for p in range(1, 49) if math.gcd(p, q) == 1 and Fraction(1, 4) <= Fraction(p, q) <= 4})


def differing(T, rate, dtype):
    """steps at which torch.arange(0, T, rate, dtype=dtype) on the CPU has another floor than (double)i * rate"""
    ar = torch.arange(0, T, rate, dtype=dtype).double()
    prod = torch.arange(len(ar), dtype=torch.float64) * rate
    return torch.nonzero(ar.floor() != prod.floor()).flatten().tolist()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the table there")
    a = ap.parse_args()
    T = a.frames
    rows = []
    for f in fractions():
        rate = f.numerator / f.denominator
        rows.append((f, rate, differing(T, rate, torch.float64), differing(T, rate, torch.float32)))
    n64, n32 = sum(1 for r in rows if r[2]), sum(1 for r in rows if r[3])
    lines = [f"torch {torch.__version__}, CPU; T = {T} frames; {len(rows)} reduced fractions p/q in [0.25, 4], q <= 24, p <= 48",
             "a step differs where floor(torch.arange(0, T, rate)[i]) != floor((double)i * rate): arange picks the neighbouring frame pair",
             f"float64 arange: {n64} of {len(rows)} rates have a differing step ({sum(len(r[2]) for r in rows)} steps in all)",
             f"float32 arange: {n32} of {len(rows)} rates have a differing step ({sum(len(r[3]) for r in rows)} steps in all)",
             f"either: {sum(1 for r in rows if r[2] or r[3])} rates; both: {sum(1 for r in rows if r[2] and r[3])} rates", "",
             "the familiar ratios:", f"{'rate':>8} {'steps':>6} {'float64: differing, first':>26} {'float32: differing, first':>26}"]

    def row(r):
        f, rate, d64, d32 = r
        cell = lambda d: f"{len(d):>6} at {d[0]:<6}" if d else f"{0:>6}    {'-':<6}"
        return f"{str(f):>8} {len(torch.arange(0, T, rate, dtype=torch.float64)):>6} {cell(d64):>26} {cell(d32):>26}"

    lines += [row(r) for r in rows if (r[0].numerator, r[0].denominator) in FAMILIAR]
    lines += ["", "the twelve rates with the most differing float64 steps:"]
    lines += [row(r) for r in sorted(rows, key=lambda r: -len(r[2]))[:12]]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
