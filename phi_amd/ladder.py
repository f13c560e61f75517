"""The sampling rule of the coverage ladder, in numpy: the test oracle of ladder.hip.

Read i (its 0-based ordinal in the order the reads reach the context) draws u_i = the upper 32 bits of output i + 1 of
SplitMix64 seeded with `seed`.  Level j of fraction f_j has the threshold t_j = min(2^32, floor(f_j * 2^32)); the band of read
i is the smallest j with u_i < t_j, or none (the read is dropped); level j = bands 0..j, so the levels are nested.  A
per-read Bernoulli draw, as `seqkit sample -p`: level sizes are not exact counts.

Nothing here touches the device or shares code with it.
"""
import math

import numpy as np

MAX_LEVELS = 16
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed, ordinals):
    """z of output number ordinal + 1 of SplitMix64(seed), uint64 (everything mod 2^64)."""
    i = np.asarray(ordinals).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (i + np.uint64(1)) * _GOLDEN
        z = (x ^ (x >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def draws(seed, ordinals):
    """u of every ordinal: the upper 32 bits of its SplitMix64 output."""
    return splitmix64(seed, ordinals) >> np.uint64(32)


def thresholds(fractions):
    """t_j = min(2^32, floor(f_j * 2^32)) in double; ValueError for a negative or decreasing fraction or a bad level count."""
    f = [float(x) for x in fractions]
    if not 1 <= len(f) <= MAX_LEVELS:
        raise ValueError(f"1 to {MAX_LEVELS} levels")
    for j, x in enumerate(f):
        if not x >= 0.0 or (j and x < f[j - 1]):
            raise ValueError(f"fraction {j} is negative or below the one before it")
    return np.array([1 << 32 if x >= 1.0 else min(1 << 32, math.floor(x * 4294967296.0)) for x in f], np.uint64)


def bands(seed, ordinals, fractions):
    """The band of every ordinal (int32); len(fractions) = dropped."""
    t = thresholds(fractions)
    return np.searchsorted(t, draws(seed, ordinals), side="right").astype(np.int32)


def level_mask(seed, ordinals, fractions, level):
    """True for the ordinals of level `level` (bands 0..level)."""
    return bands(seed, ordinals, fractions) <= level


def fractions_from_coverage(coverages, genome_size, total_bases):
    """f_j = coverage_j * genome_size / total_bases, clipped at 1 (a coverage the read set does not reach takes every read)."""
    if total_bases <= 0:
        return [1.0 for _ in coverages]
    return [min(1.0, float(cv) * float(genome_size) / float(total_bases)) for cv in coverages]
