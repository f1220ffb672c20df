"""Helper (no tests here): choose a seen-set size at which probe runs of a
given fingerprint set cross the table's end, by the host model's rules
(probe_model.py: home slot by multiply-shift on the remixed fingerprint, the
compact table's even home, linear probing).  A table that never grows has an
occupied-slot set independent of the insertion order, so the model's table is
the run's table."""
import numpy as np

import probe_model as pm

G = np.uint64(pm.G)


def remix(fps):
    with np.errstate(over="ignore"):
        return np.asarray(fps, dtype=np.uint64) * G


def mulhi(x, n):
    """floor(x * n / 2^64) for uint64 x and n < 2^32, in uint64 arithmetic."""
    assert 0 < n < 1 << 32
    n = np.uint64(n)
    s = np.uint64(32)
    return ((x >> s) * n + (((x & np.uint64(0xFFFFFFFF)) * n) >> s)) >> s


def homes(rx, nslots, compact):
    return mulhi(rx, nslots // 2) * np.uint64(2) if compact else mulhi(rx, nslots)


def carried(rx_sorted, nslots, compact):
    """Fingerprints the model places past slot nslots - 1 (they continue at
    slot 0).  rx_sorted: remixed fingerprints in ascending order (homes are
    monotone in them); exact when the array holds every fingerprint, a lower
    bound that ignores runs entering from before when it holds only a tail."""
    h = homes(rx_sorted, nslots, compact).astype(np.int64)
    idx = np.arange(len(h), dtype=np.int64)
    pos = np.maximum.accumulate(h - idx) + idx          # linear probing in home order
    return int(np.count_nonzero(pos >= nslots))


def find_size(fp_sets, compact, base=1 << 20, window=20000, want=3, tail=512):
    """The first even size >= base at which, for one of the fingerprint sets
    (one per table: the engine's, or each rank's), the model carries at least
    `want` fingerprints across the end.  Returns (size, [carried per set]);
    (None, None) when the window holds none."""
    full = [np.sort(remix(f)) for f in fp_sets]
    tails = [r[-tail:] for r in full]
    for n in range(base, base + 2 * window, 2):
        if max(carried(t, n, compact) for t in tails) < want:
            continue
        c = [carried(r, n, compact) for r in full]       # every fingerprint: exact
        if max(c) >= want:
            return n, c
    return None, None


def model_table(fps, nslots, kind):
    """The model's whole table for these fingerprints (small sets only)."""
    t = pm.Table(nslots, kind)
    for fp in fps:
        t.insert(int(fp))
    return t
