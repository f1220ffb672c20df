"""The host model of the seen-set's cold tier (cold_model.py) checked without
a GPU: its key mix against the C++ (the host path of kc_cold_key_selftest),
its set and tiering against brute force and hand-worked sequences, and the
host compile of the run search (run_find) on the clustered key sets the GPU
tests use.  test_gpu_coldset.py compares the device with this model."""
import ctypes as C

import numpy as np
import pytest

import cold_model as cm
import kubecheck
from cold_model import M64, ColdModel

U64 = np.uint64


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def test_cold_key_matches_the_host_code(oracle):
    x = cm.key_inputs(oracle)
    lib = kubecheck.load()
    k, back = np.zeros_like(x), np.zeros_like(x)
    assert lib.kc_cold_key_selftest(_u64(x), _u64(k), len(x), 0, 0) == 0
    assert lib.kc_cold_key_selftest(_u64(k), _u64(back), len(x), 1, 0) == 0
    want = [cm.cold_key(int(v)) for v in x]
    assert [int(v) for v in k] == want
    assert (back == x).all()
    assert [cm.cold_unkey(v) for v in want] == [int(v) for v in x]
    assert len(set(want)) == len({int(v) for v in x})          # a bijection on the sample
    assert lib.kc_cold_key_selftest(_u64(x), _u64(k), 0, 0, 0) == -cm.EINVAL


def test_directory_and_filter_sizes():
    assert [cm.dir_bits(n) for n in (1, 63, 64, 127, 128, 4096, 100_003)] == [1, 1, 2, 2, 3, 8, 12]
    assert cm.dir_bytes(4096) == 257 * 8
    m = ColdModel(cache_keys=False)
    assert m.add_run(np.arange(4096, dtype=U64)) == 0
    assert (m.runs[0].bits, m.runs[0].nblocks, m.meta_used) == (10, 80, 2056 + 80 * 64)
    m = ColdModel(cache_keys=False, meta_hbm_bytes=2056 + 3072)
    assert m.add_run(np.arange(4096, dtype=U64)) == 0
    assert (m.runs[0].bits, m.runs[0].nblocks) == (6, 48)
    m = ColdModel(cache_keys=False, meta_hbm_bytes=2056 + 1536)
    assert m.add_run(np.arange(4096, dtype=U64)) == 0
    assert (m.runs[0].bits, m.meta_used) == (0, 2056)
    m = ColdModel(cache_keys=False, meta_hbm_bytes=2055)
    assert m.add_run(np.arange(4096, dtype=U64)) == -cm.ENOMEM and m.failed
    m = ColdModel(cache_keys=False, bloom_bits=10)
    assert m.add_run(np.arange(3, dtype=U64)) == 0
    assert (m.runs[0].nblocks, m.meta_used) == (1, 24 + 64)


def test_tiering_by_hand():
    def sizes_after(adds, **cfg):
        m = ColdModel(cache_keys=False, **cfg)
        at, out = 0, []
        for n in adds:
            assert m.add_run(np.arange(at, at + n, dtype=U64)) == 0
            at += n
            out.append(([r.n for r in m.runs], m.merges, m.merged_keys))
        return out, m

    assert sizes_after([3000, 1999])[0][-1] == ([3000, 1999], 0, 0)
    assert sizes_after([3000, 2000])[0][-1] == ([5000], 1, 5000)
    assert sizes_after([9000, 5000, 3400])[0] == [([9000], 0, 0), ([9000, 5000], 0, 0), ([17400], 2, 8400 + 17400)]
    sizes = [20_000]
    while len(sizes) < 13:
        sizes.append(sizes[-1] * 6 // 10)
    out, m = sizes_after(sizes)
    assert [len(o[0]) for o in out] == list(range(1, 13)) + [1] and out[-1][1] == 12
    # the file tier: the oldest host run leaves first; no merge across a file run
    out, m = sizes_after([1000, 900, 800], host_bytes=7500, spill_dir=True, window_keys=64)
    assert [o[0] for o in out] == [[1000], [1000, 900], [1000, 1700]]
    assert [r.host for r in m.runs] == [False, False] and [r.nw for r in m.runs] == [16, 27]
    assert (m.host_used, m.disk_used, m.disk_written, m.merges) == (0, 2700 * 8, 2700 * 8, 1)
    m = ColdModel(cache_keys=False, host_bytes=800)
    assert m.add_run(np.arange(101, dtype=U64)) == -cm.ENOMEM and "no spill directory" in m.error


def brute_windows(keys, q, wkeys):
    """(windows read, bytes read) for a file run of sorted `keys`."""
    firsts = [0] + [keys[w] for w in range(wkeys, len(keys), wkeys)]
    read = set()
    for x in q:
        read.add(max(w for w, f in enumerate(firsts) if f <= x))
    return len(firsts) - len(read), sum(min(len(keys), (w + 1) * wkeys) - w * wkeys for w in read) * 8


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    r = cm.rng(100 + seed)
    cfg = dict(cache_keys=bool(seed & 1), merge_div=(0, 0, 4, 4, 10 ** 8, 0)[seed], bloom_bits=(10, 0, 10, 4, 10, 3)[seed])
    if seed >= 3:
        cfg.update(host_bytes=8 * 150, spill_dir=True, window_keys=64)
    m = ColdModel(**cfg)
    universe = r.sample(range(1, 6000), 3000) + [0, M64]
    r.shuffle(universe)
    have, listed, at = set(), [], 0
    for _ in range(12):
        n = r.choice((1, 2, 7, 64, 65, 100, 200))
        part = sorted(universe[at:at + n])
        at += n
        assert m.add_run(np.array(part, dtype=U64)) == 0
        have.update(part)
        listed += part
        # what holds for the runs whatever the sequence
        assert m.keys == len(listed) == sum(x.n for x in m.runs)
        assert m.host_used == 8 * sum(x.n for x in m.runs if x.host)
        assert m.disk_used == 8 * sum(x.n for x in m.runs if not x.host)
        assert len(m.runs) <= 12 or not (m.runs[-1].host and m.runs[-2].host)
        for a, b in zip(m.runs, m.runs[1:]):
            assert not (a.host and b.host) or a.n * 2 > b.n * 3
        if cfg.get("host_bytes"):
            assert m.host_used <= cfg["host_bytes"]
            assert [x.host for x in m.runs] == sorted(x.host for x in m.runs)      # files are the oldest runs
        q = sorted(set(r.sample(range(0, 6002), 300)) | {0, M64})
        pre = [int(r.random() < 0.2) for _ in q]
        files = [x for x in m.runs if not x.host and not x.cached]
        before = (m.windows_skipped, m.disk_read)
        found, hits = m.probe(np.array(q, dtype=U64), pre, hits=3)
        assert [int(f) for f in found] == [int(p or x in have) for x, p in zip(q, pre)]
        assert hits == 3 + sum(1 for x, p in zip(q, pre) if not p and x in have)
        want = [brute_windows([int(k) for k in x.keys], q, 64) for x in files]
        assert (m.windows_skipped - before[0], m.disk_read - before[1]) == (sum(w[0] for w in want), sum(w[1] for w in want))
        assert [int(k) for k in m.all_keys()] == sorted(listed)
    if not cfg["bloom_bits"] >= 4:
        assert m.filter_tests == 0


CLUSTERED = ("cluster", "mixed", "low", "high", "mid")


@pytest.mark.parametrize("shape", CLUSTERED)
def test_run_search_on_clustered_keys(shape):
    """run_find compiled for the host, on the key shapes of the GPU tests:
    found iff present, whole-run and through windows of 64, 72 and 128 keys."""
    lib = kubecheck.load()
    r = cm.rng(7)
    for n in (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000, 4096):
        keys = cm.shape_keys(shape, n, r)
        q = cm.standard_queries(keys, r)
        want = np.isin(q, keys).astype(np.uint8)
        for window in (0, 64, 72, 128):
            views = np.full(len(q), 9, dtype=np.uint8)
            assert lib.kc_cold_find_keys_selftest(_u64(keys), n, _u64(q), len(q), window,
                                                  views.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
            assert (views == want).all(), (shape, n, window)


def test_harnesses_refuse_bad_arguments_without_a_gpu():
    lib = kubecheck.load()
    a = np.array([3, 2, 1], dtype=U64)
    v = np.zeros(3, dtype=np.uint8)
    assert lib.kc_cold_find_keys_selftest(_u64(a), 3, _u64(a), 3, 0, v.ctypes.data_as(C.POINTER(C.c_uint8))) == -cm.EINVAL
    h = C.c_void_p()
    assert lib.kc_coldset_create(0, 0, None, 60, 10, 1, 0, 16, C.byref(h)) == -cm.EINVAL
    assert lib.kc_coldset_add_run(None, _u64(a), 3) == -cm.EINVAL
    assert lib.kc_coldset_probe(None, _u64(a), 3, None, None) == -cm.EINVAL
    assert lib.kc_spill_selftest(4, 1, None, 0, None, 0, None, 0, 0, None, 0, None) == -cm.EINVAL
    assert lib.kc_spill_selftest(0, 3, None, 0, None, 0, None, 0, 0, None, 0, None) == -cm.EINVAL
