"""CPU tests of the host model of the seen-set tables (tests/probe_model.py),
the reference tests/test_gpu_probe.py and test_gpu_table_edges.py compare the
device probe loops with."""
import pytest

import probe_model as pm
from probe_model import CL_CUR, CL_FULL, CL_LOST, CL_NEW, CL_OLD, Table


def test_home_spot_values():
    # fp * G mod 2^64 / 2^64 for fp = 1, 2, 3 is frac(k * 0.6180339887...) =
    # 0.618034, 0.236068, 0.854102; the home is floor(that * buckets)
    for fp, frac in ((1, 0.6180339887), (2, 0.2360679775), (3, 0.8541019662)):
        for n in (64, 66, 1 << 20):
            assert pm.home(fp, n, "wide") == pm.home(fp, n, "fpset") == int(frac * n)
            assert pm.home(fp, n, "compact") == 2 * int(frac * (n // 2))
    assert [pm.home(fp, 64, "wide") for fp in (1, 2, 3)] == [39, 15, 54]
    assert [pm.home(fp, 66, "wide") for fp in (1, 2, 3)] == [40, 15, 56]
    assert [pm.home(fp, 64, "compact") for fp in (1, 2, 3)] == [38, 14, 54]
    assert [pm.home(fp, 66, "compact") for fp in (1, 2, 3)] == [40, 14, 56]
    # the top (owner) bits alone do not pick the bucket
    assert pm.home(1 | 5 << 59, 64, "wide") != pm.home(1 | 6 << 59, 64, "wide")
    # LDS: the low 32 bits only
    assert pm.home(0x7123456700000805, pm.LDS_NT, "lds") == 5
    assert pm.home(0x7123456780000000, pm.LDS_NT_SH, "lds") == 896
    assert pm.home(0x71234567FFFFFFFF, pm.LDS_NT_SH, "lds") == 1791
    assert pm.home(0x7123456700000805, pm.LDS_NT_SH, "lds") == 0


@pytest.mark.parametrize("kind", ["wide", "compact", "fpset", "lds"])
def test_craft_homes(kind):
    rng = pm.rng(1)
    sizes = (pm.LDS_NT, pm.LDS_NT_SH) if kind == "lds" else (8, 16, 64, 72) if kind == "fpset" else (4, 8, 16, 64, 66, 1 << 20)
    for n in sizes:
        for slot in (0, n - 2, n - 1):
            if kind == "compact" and slot & 1:
                continue
            fps = pm.craft(slot, n, kind, 20, rng)
            assert len(set(fps)) == 20 and all(0 < f < 1 << 63 for f in fps)
            assert {pm.home(f, n, kind) for f in fps} == {slot}


@pytest.mark.parametrize("kind,n", [("wide", 66), ("compact", 66), ("fpset", 72), ("wide", 16), ("compact", 16)])
def test_occupied_slots_independent_of_order(kind, n):
    # a wrap case: homes in the last slots and the first, the table 2/3 full
    rng = pm.rng(2)
    last = n - 2 if kind == "compact" else n - 1
    fps = (pm.craft(last, n, kind, n // 3, rng) + pm.craft(0, n, kind, n // 6, rng) +
           pm.craft(n - 2, n, kind, n // 6, rng))
    fps = list(dict.fromkeys(fps))
    ref = None
    for _ in range(1000):
        rng.shuffle(fps)
        t = Table(n, kind)
        for fp in fps:
            assert t.insert(fp) == CL_NEW
        t.check_runs()
        occ = t.occupied()
        assert ref is None or occ == ref
        ref = occ
    assert 0 in ref and last in ref and len(ref) == len(fps)     # the run crossed the end
    # the pipelined group order of k_claim fills the same slots
    if kind == "compact":
        t = Table(n, kind)
        res = []
        for k in range(0, len(fps), pm.CLAIM_BATCH):
            res += t.pair_group(fps[k:k + pm.CLAIM_BATCH])
        assert res == [CL_NEW] * len(fps) and t.occupied() == ref
        t.check_runs()


def test_wrap_and_full_table():
    rng = pm.rng(3)
    for kind, n in (("wide", 4), ("compact", 4), ("fpset", 8), ("wide", 66), ("compact", 66)):
        last = n - 2 if kind == "compact" else n - 1
        fps = pm.craft(last, n, kind, n + 1, rng)
        t = Table(n, kind)
        assert [t.insert(f) for f in fps[:n]] == [CL_NEW] * n
        # the run continues at slot 0
        assert t.fp_at(last) == fps[0] and t.fp_at(0) == fps[2 if kind == "compact" else 1]
        img = list(t.w)
        assert t.insert(fps[n]) == CL_FULL and t.w == img          # full: refused, unchanged
        assert all(t.insert(f) == CL_OLD for f in fps[:n])          # present at 100 % load
        assert t.contains(fps[n]) == 0
        if kind == "compact":
            assert t.pair_insert(fps[n]) == CL_FULL and t.pair_group([fps[n], fps[0]]) == [CL_FULL, CL_OLD]


def test_claim_order_rule():
    # claim = level << 44 | key: the smallest claim of the level wins, earlier levels are old
    t = Table(8, "wide")
    fp = pm.craft(7, 8, "wide", 1, pm.rng(4))[0]
    assert t.claim(fp, 9, 5) == CL_NEW and t.get(fp) == pm.nclaim(5, 9)
    assert t.claim(fp, 12, 5) == CL_LOST and t.claim(fp, 9, 5) == CL_LOST
    assert t.claim(fp, 3, 5) == CL_CUR and t.get(fp) == pm.nclaim(5, 3)
    assert t.claim(fp, 0, 6) == CL_OLD and t.get(fp) == pm.nclaim(5, 3)
    # the STORE-claim protocol: candidates write nothing in the claim launch
    t = Table(8, "wide")
    codes, holds = t.store_protocol([fp, fp, fp, fp], [9, 3, 12, 5], 5)
    assert codes == [CL_NEW, CL_CUR, CL_LOST, CL_CUR] and holds == [0, 1, 0, 0]
    assert t.get(fp) == pm.nclaim(5, 3)
    # a claim word of 0 (first-claim insert) is pending, current level
    t = Table(8, "wide")
    assert t.insert(fp) == CL_NEW and t.get(fp) == 0
    assert t.claim(fp, 7, 2, store=False) == CL_CUR


def test_pair_group_order():
    # two fingerprints of one home in one group: the first CAS wins the home
    # slot, the second carries on in home + 1
    a, b = pm.craft(6, 8, "compact", 2, pm.rng(5))
    t = Table(8, "compact")
    assert t.pair_group([a, b]) == [CL_NEW, CL_NEW] and t.w[6:8] == [a, b]
    assert t.pair_group([b, a]) == [CL_OLD, CL_OLD]
    c, d = pm.craft(6, 8, "compact", 4, pm.rng(5))[2:]
    assert t.pair_group([c, d]) == [CL_NEW, CL_NEW] and t.w[0:2] == [c, d]    # past the pair: slot 0


def test_rehash_model():
    rng = pm.rng(6)
    t = Table(16, "wide")
    for k, fp in enumerate(pm.craft(15, 16, "wide", 6, rng)):
        t.claim(fp, k, 3)
    for n in (32, 38):
        nw = pm.rehash(t, n)
        assert nw.fps() == t.fps()
        assert all(nw.get(fp) == t.get(fp) for fp in t.fps())
        nw.check_runs()


def test_carried_across_the_end_matches_the_table():
    # table_edge_search.carried (vectorised, by sorted home) against the model's table
    import numpy as np
    import table_edge_search as tes
    rng = pm.rng(7)
    for compact, kind in ((False, "wide"), (True, "compact")):
        for n in (64, 66, 130):
            last = n - 2 if compact else n - 1
            for extra in (0, 3, 9):
                fps = [rng.getrandbits(63) | 1 for _ in range(n // 4)] + pm.craft(last, n, kind, extra, rng) + \
                    pm.craft(n - 4, n, kind, extra // 3, rng)
                rx = np.sort(tes.remix(fps))
                assert [int(h) for h in tes.homes(rx, n, compact)] == sorted(pm.home(f, n, kind) for f in fps)
                t = tes.model_table(fps, n, kind)
                # what is carried in from the end takes the first slots
                c = tes.carried(rx, n, compact)
                assert c >= max(0, extra - (2 if compact else 1))
                assert set(range(c)) <= t.occupied() and len(t.occupied()) == len(fps)
    assert tes.find_size([[rng.getrandbits(63) | 1 for _ in range(2000)]], False, base=6002, window=50) == (None, None)
    dense = pm.craft(6099, 6100, "wide", 4, rng) + [rng.getrandbits(63) | 1 for _ in range(100)]
    n, c = tes.find_size([dense], False, base=6000, window=100)
    assert n is not None and n <= 6100 and c[0] >= 3
