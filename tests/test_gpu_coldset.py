"""The seen-set's cold tier driven directly: kc_coldset_* runs a kc::ColdSet
(coldset.hip: k_run_meta, k_cold_probe, k_cold_merge_probe, k_window_ranges,
the host merge, the file tier, the HBM key cache) on runs and query sets made
here, and every found byte, the hit counter, all_keys and the statistics are
compared with the host model (cold_model.py) after every call.  Integers
only: every comparison is exact, except that of filter_passed (the Bloom hash
is not modelled) the tests hold
    hits found in filtered runs <= filter_passed <= filter_tests.
KC_COLD_MERGE_DIV must be unset (ColdSet::init reads it)."""
import ctypes as C
import os

import numpy as np
import pytest

import cold_model as cm
import kubecheck
from cold_model import M64, ColdModel

pytestmark = pytest.mark.gpu

U64 = np.uint64
SMALL = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65)
SIZES = SMALL + (127, 128, 129, 4096)
SHAPES = ("uniform", "low", "high", "mid", "cluster", "mixed")


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Both:
    """One ColdSet on the device and its model, given the same calls; every
    call compares the answers and then the statistics."""

    def __init__(self, spill_dir=None, **cfg):
        assert "KC_COLD_MERGE_DIV" not in os.environ
        self.lib = kubecheck.load()
        self.m = ColdModel(spill_dir=spill_dir is not None, **cfg)
        d = dict(meta_hbm_bytes=0, host_bytes=0, window_keys=1 << 23, bloom_bits=10, cache_keys=True, merge_div=0,
                 merge_threads=16)
        d.update(cfg)
        self.h = C.c_void_p()
        kubecheck._lib.check("kc_coldset_create", self.lib.kc_coldset_create(
            d["meta_hbm_bytes"], d["host_bytes"], str(spill_dir).encode() if spill_dir is not None else None,
            d["window_keys"], d["bloom_bits"], int(d["cache_keys"]), d["merge_div"], d["merge_threads"],
            C.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.kc_coldset_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def error(self):
        return self.lib.kc_last_error().decode()

    def dev_stats(self):
        out = np.zeros(len(cm.STATS), dtype=U64)
        assert self.lib.kc_coldset_stats(self.h, _u64(out)) == 0
        return dict(zip(cm.STATS, (int(x) for x in out)))

    def check_stats(self):
        got, want = self.dev_stats(), self.m.stats()
        assert {k: got[k] for k in cm.EXACT} == want
        assert self.m.filtered_hits <= got["filter_passed"] <= got["filter_tests"]
        return got

    def add(self, keys, want=0):
        keys = np.ascontiguousarray(keys, dtype=U64)
        rc = self.lib.kc_coldset_add_run(self.h, _u64(keys), len(keys))
        assert rc == self.m.add_run(keys) == want, self.error()
        if rc == 0:
            self.check_stats()
        else:
            assert self.m.error in self.error()
        return rc

    def dev_probe(self, q, found, hits):
        q = np.ascontiguousarray(q, dtype=U64)
        f = np.array(found, dtype=np.uint8)
        h = np.array([hits], dtype=U64)
        rc = self.lib.kc_coldset_probe(self.h, _u64(q), len(q), _u8(f), _u64(h))
        return rc, f, int(h[0])

    def probe(self, q, found=None, hits=0):
        """Probe on both; (found bytes, hits), equal on both sides."""
        q = np.ascontiguousarray(q, dtype=U64)
        found = np.zeros(len(q), dtype=np.uint8) if found is None else np.array(found, dtype=np.uint8)
        rc, f, h = self.dev_probe(q, found, hits)
        assert rc == 0, self.error()
        wf, wh = self.m.probe(q, found, hits)
        bad = np.nonzero(f != wf)[0]
        assert len(bad) == 0, [(int(i), hex(int(q[i])), int(f[i]), int(wf[i])) for i in bad[:8]]
        assert h == wh
        self.check_stats()
        return f, h

    def all_keys(self):
        want = self.m.all_keys()
        out = np.zeros(max(1, len(want)), dtype=U64)
        n = self.lib.kc_coldset_all_keys(self.h, _u64(out), len(out))
        assert n == len(want), self.error()
        assert (out[:n] == want).all()
        self.check_stats()
        return want

    def clear(self):
        assert self.lib.kc_coldset_clear(self.h) == 0
        self.m.clear()
        got = self.check_stats()
        assert not any(got.values())


def present(keys, q):
    return np.isin(np.asarray(q, dtype=U64), np.asarray(keys, dtype=U64)).astype(np.uint8)


def full_check(b, keys, r, extra=300, slices=True):
    """The standard queries, whole and in slices of 1, 63, 64 and 65 (partial
    waves for the ballots); then all_keys.  `keys`: every key added."""
    q = cm.standard_queries(keys, r, extra)
    f, h = b.probe(q)
    want = present(keys, q)
    assert (f == want).all() and h == int(want.sum())       # (the model's answer, said again in plain words)
    if slices:
        for w in (1, 63, 64, 65):
            for at in sorted({0, max(0, len(q) // 2 - w // 2), max(0, len(q) - w)}):
                b.probe(q[at:at + w])
    b.all_keys()


# ------------------------------------------------------------------ key shapes and run sizes
@pytest.mark.parametrize("cache", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_sizes(shape, cache):
    r = cm.rng(SHAPES.index(shape) * 2 + cache)
    for n in SIZES + ((100_003,) if shape == "uniform" else ()):
        keys = cm.shape_keys(shape, n, r)
        with Both(cache_keys=cache) as b:
            b.add(keys)
            s = b.check_stats()
            assert (s["cached_runs"], s["cache_bytes"]) == ((1, n * 8) if cache else (0, 0))
            full_check(b, keys, r)


def test_cache_and_host_reads_agree():
    r = cm.rng(5)
    for shape in SHAPES:
        keys = cm.shape_keys(shape, 1000, r)
        q = cm.standard_queries(keys, r)
        res = []
        for cache in (0, 1):
            with Both(cache_keys=cache) as b:
                b.add(keys)
                res.append(b.probe(q))
        assert (res[0][0] == res[1][0]).all() and res[0][1] == res[1][1]


# ------------------------------------------------------------------ filters
@pytest.mark.parametrize("bloom_bits", [10, 4, 3, 0])
def test_filters_lose_no_key(bloom_bits):
    r = cm.rng(bloom_bits + 11)
    for shape in SHAPES:
        for n in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4096):
            keys = cm.shape_keys(shape, n, r)
            with Both(bloom_bits=bloom_bits, cache_keys=0) as b:
                b.add(keys)
                assert b.m.runs[0].bits == (bloom_bits if bloom_bits >= 4 else 0)
                f, h = b.probe(keys)
                assert f.all() and h == n
                full_check(b, keys, r, slices=False)
                s = b.check_stats()
                assert (s["filter_tests"] > 0) == (bloom_bits >= 4)


@pytest.mark.parametrize("shape", ["uniform", "cluster"])
def test_filter_bits_from_the_budget(shape):
    r = cm.rng(23)
    n = 4096
    keys = cm.shape_keys(shape, n, r)
    for bits in (6, 3):
        with Both(meta_hbm_bytes=cm.dir_bytes(n) + bits * n // 8, cache_keys=0) as b:
            b.add(keys)
            assert b.m.runs[0].bits == (bits if bits >= 4 else 0)
            assert b.check_stats()["meta_bytes"] == cm.dir_bytes(n) + (bits * n // 512 * 64 if bits >= 4 else 0)
            full_check(b, keys, r)
            assert (b.check_stats()["filter_tests"] > 0) == (bits >= 4)


def test_key_copies_within_the_budget():
    # 38,000 B for directories, filters and key copies: the copies are made newest first as room allows, and the
    # fourth run's directory and filter push the oldest copy (24,000 B) out, which lets the second run's in
    r = cm.rng(27)
    parts = split(cm.shape_keys("uniform", 5500, r), (3000, 1500, 700, 300), r)
    with Both(meta_hbm_bytes=38_000, cache_keys=1) as b:
        have = np.zeros(0, dtype=U64)
        for p, (cached, cache_bytes) in zip(parts, [(1, 24_000), (1, 24_000), (2, 29_600), (3, 20_000)]):
            b.add(p)
            s = b.check_stats()
            assert (s["cached_runs"], s["cache_bytes"]) == (cached, cache_bytes)
            assert s["meta_bytes"] + s["cache_bytes"] <= s["peak_meta_bytes"] <= 38_000
            have = np.sort(np.concatenate([have, p]))
            full_check(b, have, r)
        assert b.check_stats()["runs"] == 4


def test_directory_does_not_fit():
    r = cm.rng(29)
    n = 4096
    keys = cm.shape_keys("uniform", n, r)
    with Both(meta_hbm_bytes=cm.dir_bytes(n) - 1, cache_keys=0) as b:
        assert b.add(keys, want=-cm.ENOMEM) == -12
        assert "HBM budget for cold-run directories exhausted" in b.error()
        # the set holds a run without a directory: the harness refuses to probe it
        rc, _, _ = b.dev_probe(keys[:4], np.zeros(4, dtype=np.uint8), 0)
        assert rc == -cm.EINVAL
        out = np.zeros(4, dtype=U64)
        assert b.lib.kc_coldset_all_keys(b.h, _u64(out), 4) == -cm.EINVAL
        assert b.lib.kc_coldset_add_run(b.h, _u64(keys), 4) == -cm.EINVAL
        b.clear()
        small = cm.shape_keys("uniform", 40, r)       # (a 3-entry directory fits)
        b.add(small)
        full_check(b, small, r)


# ------------------------------------------------------------------ file tier
FILE_LENGTHS = (64, 65, 71, 72, 127, 128, 129, 1000)
W = 64


def window_queries(keys):
    """Query sets placed on the windows of a file run of `keys` (W keys each)."""
    n = len(keys)
    k = [int(x) for x in keys]
    firsts = [k[w] for w in range(0, n, W)]
    lasts = [k[min(n, w + W) - 1] for w in range(0, n, W)]
    sets = {
        "firsts and one below": {x for f in firsts for x in (f, (f - 1) & M64)},
        "lasts": set(lasts),
        "only the top word": {M64},
    }
    nw = len(firsts)
    w = nw // 2
    lo, hi = w * W, min(n, w * W + W)
    inside = set(k[lo:hi][:10]) | {(a + b) // 2 for a, b in zip(k[lo:hi - 1], k[lo + 1:hi])}
    sets["inside one window"] = inside
    if nw > 1:
        sets["none below window 1"] = set(k[W:W + 20]) | {min(k[W] + 1, M64), M64}
    return {name: cm.u64(s) for name, s in sets.items()}, w, hi - lo


@pytest.mark.parametrize("cache", [0, 1])
@pytest.mark.parametrize("shape", ["uniform", "low", "high"])
def test_file_tier(tmp_path, shape, cache):
    r = cm.rng(31 + cache)
    for n in FILE_LENGTHS:
        keys = cm.shape_keys(shape, n, r)
        nw = -(-n // W)
        b = Both(spill_dir=tmp_path, host_bytes=8, window_keys=W, cache_keys=cache)
        b.add(keys)
        s = b.check_stats()
        assert (s["runs"], s["runs_disk"], s["host_bytes"], s["disk_bytes"], s["disk_written"]) == (1, 1, 0, n * 8, n * 8)
        assert len(os.listdir(tmp_path)) == 1
        # (with the cache the add streamed the file back into HBM, and probes read the copy)
        assert (s["cached_runs"], s["disk_read"]) == ((1, n * 8) if cache else (0, 0))
        sets, w, wlen = window_queries(keys)
        for name, q in sets.items():
            before = b.dev_stats()
            f, h = b.probe(q)
            assert (f == present(keys, q)).all(), name
            after = b.dev_stats()
            read, skipped = after["disk_read"] - before["disk_read"], after["windows_skipped"] - before["windows_skipped"]
            if cache:
                assert (read, skipped) == (0, 0), name
            elif name == "inside one window":
                assert (read, skipped) == (wlen * 8, nw - 1), name
            elif name == "none below window 1":
                assert skipped >= 1 and read <= (n - W) * 8, name
            elif name == "only the top word":
                assert (read, skipped) == ((n - (nw - 1) * W) * 8, nw - 1), name
        full_check(b, keys, r)
        b.close()
        assert os.listdir(tmp_path) == []


def test_file_tier_several_runs(tmp_path):
    # three file runs and a host run, probed together; then the set with HBM copies
    r = cm.rng(37)
    for cache in (0, 1):
        allk = cm.shape_keys("uniform", 1000 + 600 + 129 + 50, r)
        parts = split(allk, (1000, 600, 129, 50), r)
        with Both(spill_dir=tmp_path, host_bytes=8 * 100, window_keys=W, cache_keys=cache) as b:
            for p in parts:
                b.add(p)
            s = b.check_stats()
            assert (s["runs"], s["runs_disk"], s["merges"]) == (4, 3, 0)
            full_check(b, allk, r)
        assert os.listdir(tmp_path) == []


def test_no_spill_directory():
    r = cm.rng(41)
    with Both(host_bytes=8 * 100, cache_keys=0) as b:
        b.add(cm.shape_keys("uniform", 100, r))                 # fits
        b.clear()
        assert b.add(cm.shape_keys("uniform", 101, r), want=-cm.ENOMEM) == -12
        assert "no spill directory" in b.error()


# ------------------------------------------------------------------ streaming merge-probe
MERGE_LENGTHS = (1, 2047, 2048, 2049, 4096, 4097)


def segment_queries(keys):
    k = [int(x) for x in keys]
    s = set()
    for s0 in range(0, len(k), cm.MSEG):
        for e in (k[s0], k[min(len(k), s0 + cm.MSEG) - 1]):
            s.update((e, (e - 1) & M64, (e + 1) & M64))
    return cm.u64(s)


@pytest.mark.parametrize("shape", ["uniform", "high", "low"])
def test_merge_probe(shape):
    r = cm.rng(43)
    for n in MERGE_LENGTHS:
        keys = cm.shape_keys(shape, n, r)
        with Both(merge_div=10 ** 8, cache_keys=0) as b:
            b.add(keys)
            q = segment_queries(keys)
            f, h = b.probe(q)
            assert (f == present(keys, q)).all()
            if n > cm.MSEG and int(keys[cm.MSEG]) - int(keys[cm.MSEG - 1]) > 2:
                # a query set wholly between two segments
                lo, hi = int(keys[cm.MSEG - 1]), int(keys[cm.MSEG])
                f, h = b.probe(cm.u64({lo + 1, (lo + hi) // 2, hi - 1}))
                assert not f.any() and h == 0
            full_check(b, keys, r)
            s = b.check_stats()
            assert s["filter_tests"] == 0 and s["merge_probes"] == b.m.merge_probes > 0


def test_merge_probe_some_runs():
    r = cm.rng(47)
    allk = cm.shape_keys("uniform", 4096 + 1000, r)
    big, small = split(allk, (4096, 1000), r)
    with Both(merge_div=8, cache_keys=0) as b:
        b.add(big)
        b.add(small)                       # under 2/3 of the first: two runs
        assert b.check_stats()["runs"] == 2
        q = cm.standard_queries(allk, r)
        for m, want in ((50, 0), (200, 1), (600, 2)):   # merge-probed: runs with n / 8 <= m
            before = b.dev_stats()["merge_probes"]
            sub = q[::len(q) // m][:m]
            f, h = b.probe(sub)
            assert (f == present(allk, sub)).all()
            assert b.dev_stats()["merge_probes"] - before == want
        full_check(b, allk, r)


# ------------------------------------------------------------------ tiering and merges
def split(allk, sizes, r):
    """Disjoint sorted key sets of the given sizes out of allk."""
    perm = np.array(r.sample(range(len(allk)), sum(sizes)))
    out, at = [], 0
    for n in sizes:
        out.append(np.sort(allk[perm[at:at + n]]))
        at += n
    return out


def add_all(b, parts, r, expect):
    """Add the parts; after each, (runs, merges, merged_keys) are as given
    (and the model's), all_keys is the sorted union and every key is found."""
    have = np.zeros(0, dtype=U64)
    for p, e in zip(parts, expect):
        b.add(p)
        s = b.check_stats()
        assert (s["runs"], s["merges"], s["merged_keys"]) == e
        have = np.sort(np.concatenate([have, p]))
        assert (b.all_keys() == have).all()
        f, h = b.probe(have)
        assert f.all() and h == len(have)
    return have


@pytest.mark.parametrize("cache", [0, 1])
def test_tiering(cache):
    r = cm.rng(53)
    allk = cm.shape_keys("uniform", 40_000, r)
    # under 2/3: no merge; exactly 2/3: merge
    with Both(cache_keys=cache) as b:
        add_all(b, split(allk, (3000, 1999), r), r, [(1, 0, 0), (2, 0, 0)])
    with Both(cache_keys=cache) as b:
        add_all(b, split(allk, (3000, 2000), r), r, [(1, 0, 0), (1, 1, 5000)])
    # a cascade: 5000 + 3400 merge (10000 <= 10200), then 9000 + 8400 (18000 <= 25200)
    with Both(cache_keys=cache) as b:
        have = add_all(b, split(allk, (9000, 5000, 3400), r), r, [(1, 0, 0), (2, 0, 0), (1, 2, 8400 + 17400)])
        full_check(b, have, r, slices=False)


def test_more_than_twelve_runs():
    r = cm.rng(59)
    sizes = [20_000]
    while len(sizes) < 13:
        sizes.append(sizes[-1] * 6 // 10)
    assert all(a * 2 > b * 3 for a, b in zip(sizes, sizes[1:]))
    allk = cm.shape_keys("uniform", sum(sizes), r)
    expect = [(i + 1, 0, 0) for i in range(12)]
    merged, acc = 0, 0
    for n in reversed(sizes):              # the 13th run trips the rule, and the cascade ends in one run
        acc += n
        merged += acc if acc > n else 0
    expect.append((1, 12, merged))
    with Both(cache_keys=0) as b:
        have = add_all(b, split(allk, sizes, r), r, expect)
        full_check(b, have, r, slices=False)


def big_keys(n, r, lo=0, hi=1 << 64):
    g = np.random.default_rng(r.getrandbits(32))
    out = np.zeros(0, dtype=U64)
    while len(out) < n:
        more = g.integers(0, hi - lo, size=n, dtype=U64, endpoint=False) + U64(lo)
        out = np.unique(np.concatenate([out, more]))
    return np.sort(g.permutation(out)[:n])


@pytest.mark.parametrize("case", ["low+high", "high+low"])
def test_merge_two_ranges(case):
    # 70,000 merged keys: 2 thread ranges, each holding one whole run
    r = cm.rng(61)
    lo, hi = big_keys(40_000, r, 0, 1 << 63), big_keys(30_000, r, 1 << 63, 1 << 64)
    if case == "high+low":
        lo, hi = big_keys(40_000, r, 1 << 63, 1 << 64), big_keys(30_000, r, 0, 1 << 63)
    assert cm.merge_ranges(70_000, 16) == 2
    with Both(cache_keys=0) as b:
        add_all(b, [lo, hi], r, [(1, 0, 0), (1, 1, 70_000)])
        assert b.m.merge_range_log == [2]
        full_check(b, np.concatenate([lo, hi]), r, slices=False)


@pytest.mark.parametrize("case", ["uniform", "top sixteenth"])
def test_merge_sixteen_ranges(case):
    r = cm.rng(67)
    lo = 0 if case == "uniform" else 15 << 60     # (top sixteenth: 15 of the 16 ranges hold no key)
    allk = big_keys(1_000_000, r, lo, 1 << 64)
    g = np.random.default_rng(1)
    pick = np.zeros(len(allk), dtype=bool)
    pick[g.permutation(len(allk))[:500_000]] = True
    assert cm.merge_ranges(1_000_000, 16) == 16
    with Both(cache_keys=0) as b:
        b.add(allk[pick])
        b.add(allk[~pick])
        s = b.check_stats()
        assert (s["runs"], s["merges"], s["merged_keys"]) == (1, 1, 1_000_000)
        assert (b.all_keys() == allk).all()
        f, h = b.probe(allk)
        assert f.all() and h == len(allk)
        q = np.unique(np.concatenate([allk[::97] + U64(1), allk[::89] - U64(1), np.array([0, M64, 1 << 63], dtype=U64)]))
        f, h = b.probe(q)
        assert (f == present(allk, q)).all()


def test_no_merge_across_a_file_run(tmp_path):
    # 1000 keys go to a file; 900 more (which two host runs would merge with them) stay apart
    r = cm.rng(71)
    a, c, d = split(cm.shape_keys("uniform", 2700, r), (1000, 900, 800), r)
    with Both(spill_dir=tmp_path, host_bytes=7500, window_keys=W, cache_keys=0) as b:
        b.add(a)
        s = b.check_stats()
        assert (s["runs"], s["runs_disk"]) == (1, 1)
        b.add(c)
        s = b.check_stats()
        assert (s["runs"], s["runs_disk"], s["merges"]) == (2, 1, 0)
        full_check(b, np.concatenate([a, c]), r)
        b.add(d)                           # the two host runs merge, and the result goes to a second file
        s = b.check_stats()
        assert (s["runs"], s["runs_disk"], s["merges"], s["merged_keys"]) == (2, 2, 1, 1700)
        full_check(b, np.concatenate([a, c, d]), r)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("sizes", [(3000, 1000), (3000, 2500)])
def test_same_key_in_two_runs(sizes):
    # (the engine never does this) apart or merged: found once, listed twice
    r = cm.rng(73)
    a, c = split(cm.shape_keys("uniform", sum(sizes), r), sizes, r)
    dup = a[len(a) // 2]
    c = np.unique(np.concatenate([c, [dup]]))
    with Both(cache_keys=0) as b:
        b.add(a)
        b.add(c)
        assert b.check_stats()["runs"] == (2 if sizes[1] == 1000 else 1)
        f, h = b.probe(np.array([dup], dtype=U64), hits=5)
        assert f[0] == 1 and h == 6
        allk = b.all_keys()
        assert int((allk == dup).sum()) == 2 and len(allk) == len(a) + len(c)
        q = cm.standard_queries(np.concatenate([a, c]), r)
        f, h = b.probe(q)
        assert h == int(f.sum()) == len(a) + len(c) - 1


# ------------------------------------------------------------------ found / hits semantics, reuse, arguments
@pytest.mark.parametrize("cfg", [dict(cache_keys=0), dict(cache_keys=1), dict(cache_keys=0, merge_div=10 ** 8)])
def test_found_and_hits_semantics(cfg):
    r = cm.rng(79)
    keys = cm.shape_keys("uniform", 3000, r)
    q = cm.standard_queries(keys, r)
    want = present(keys, q)
    with Both(**cfg) as b:
        b.add(keys)
        pre = np.array([r.random() < 0.3 for _ in q], dtype=np.uint8)      # present and absent ones
        before = b.dev_stats()["filter_tests"]
        f, h = b.probe(q, found=pre, hits=1000)
        assert (f == (pre | want)).all()
        assert h == 1000 + int((want & ~pre & 1).sum())
        if not cfg.get("merge_div"):
            assert b.dev_stats()["filter_tests"] - before == int((pre == 0).sum())
        f, h = b.probe(q, found=np.ones(len(q), dtype=np.uint8), hits=7)
        assert f.all() and h == 7
        # clear, then the same handle as a fresh one
        b.clear()
        keys2 = cm.shape_keys("mixed", 500, r)
        b.add(keys2)
        full_check(b, keys2, r)


def test_harness_refuses_bad_arguments():
    r = cm.rng(83)
    keys = cm.shape_keys("uniform", 100, r)
    with Both(cache_keys=0) as b:
        lib, h = b.lib, b.h
        f, hits = np.zeros(4, dtype=np.uint8), np.zeros(1, dtype=U64)
        for bad in (keys[::-1].copy(), np.array([5, 5], dtype=U64), np.array([3, 9, 8], dtype=U64)):
            assert lib.kc_coldset_add_run(h, _u64(bad), len(bad)) == -cm.EINVAL
            assert "strictly ascending" in b.error()
        assert lib.kc_coldset_add_run(h, _u64(keys), 0) == -cm.EINVAL
        assert lib.kc_coldset_add_run(h, _u64(keys), (1 << 21) + 1) == -cm.EINVAL       # (refused before any read)
        b.add(keys)
        bad = np.array([9, 3, 4, 5], dtype=U64)
        assert lib.kc_coldset_probe(h, _u64(bad), 4, _u8(f), _u64(hits)) == -cm.EINVAL
        assert "not ascending" in b.error()
        assert lib.kc_coldset_probe(h, _u64(bad), 0, _u8(f), _u64(hits)) == -cm.EINVAL
        assert lib.kc_coldset_probe(h, _u64(bad), (1 << 21) + 1, _u8(f), _u64(hits)) == -cm.EINVAL
        assert not f.any() and hits[0] == 0
        full_check(b, keys, r)             # and the set is as it was
    hh = C.c_void_p()
    assert kubecheck.load().kc_coldset_create(0, 0, None, 63, 10, 1, 0, 16, C.byref(hh)) == -cm.EINVAL


# ------------------------------------------------------------------ the key mix on the device
def test_cold_key_on_the_device(oracle):
    x = cm.key_inputs(oracle)
    lib = kubecheck.load()
    k, back = np.zeros_like(x), np.zeros_like(x)
    assert lib.kc_cold_key_selftest(_u64(x), _u64(k), len(x), 0, 1) == 0
    assert lib.kc_cold_key_selftest(_u64(k), _u64(back), len(x), 1, 1) == 0
    assert [int(v) for v in k] == [cm.cold_key(int(v)) for v in x]
    assert (back == x).all()
