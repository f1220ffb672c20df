"""The checkpoint streams on the device, through kc_ckpt_selftest, against the
host model of the tables (probe_model.Table): k_ckpt_pack over crafted table
images in windows, and the recovery's list inserts into an empty table.
Integers only: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import ckpt_model as cm
import kubecheck
import probe_model as pm
from probe_model import Table

pytestmark = pytest.mark.gpu

KIND = {0: "wide", 1: "compact"}
STAGE = 4096          # the smallest staging buffer: 512 words


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def pack(layout, image, nslots, window, stage=STAGE):
    """k_ckpt_pack over `image`: (stream, [count, sum, xor, received])."""
    lib = kubecheck.load()
    t = np.array(image, dtype=np.uint64)
    out = np.zeros(nslots, dtype=np.uint64)
    st = np.zeros(4, dtype=np.uint64)
    kubecheck._lib.check("kc_ckpt_selftest", lib.kc_ckpt_selftest(0, layout, nslots, _u64(t), len(t), window, stage,
                                                                   _u64(out), _u64(st)))
    st = [int(x) for x in st]
    return [int(x) for x in out[:st[0]]], st


def restore(layout, fps, nslots, window, stage=STAGE):
    """The recovery's inserts of `fps` into an empty table: (image, [bad, sum, xor, n])."""
    lib = kubecheck.load()
    f = np.array(fps, dtype=np.uint64)
    out = np.zeros(nslots * (1 if layout else 2), dtype=np.uint64)
    st = np.zeros(4, dtype=np.uint64)
    kubecheck._lib.check("kc_ckpt_selftest", lib.kc_ckpt_selftest(1, layout, nslots, _u64(f) if len(f) else None,
                                                                   len(f), window, stage, _u64(out), _u64(st)))
    return [int(x) for x in out], [int(x) for x in st]


def crafted_table(layout, nslots, fill, seed):
    """A table with a run that starts at the last slot (pair) and wraps, slot 0
    and slot nslots - 1 occupied, an empty stretch of more than 8 slots, and
    `fill` entries in all (0: empty)."""
    kind = KIND[layout]
    r = pm.rng(seed)
    t = Table(nslots, kind)
    if fill == 0:
        return t
    last_home = nslots - 2 if layout else nslots - 1
    fps = pm.craft(last_home, nslots, kind, 4, r)           # fills the last slot(s) and wraps over slot 0
    # the rest at homes in the first third and the last sixth: the middle stays empty
    homes = list(range(2, nslots // 3)) + list(range(nslots - nslots // 6, nslots))
    while len(fps) < fill:
        h = r.choice(homes)
        fps += pm.craft(h & ~1 if layout else h, nslots, kind, 1, r)    # (a compact home is an even slot)
    for k, fp in enumerate(fps[:fill]):
        if layout:
            assert t.pair_insert(fp) == pm.CL_NEW
        else:
            assert t.claim(fp, k, 3) == pm.CL_NEW
    assert t.fp_at(0) and t.fp_at(nslots - 1)
    assert not any(t.fp_at(i) for i in range(nslots // 2 - 5, nslots // 2 + 5))
    return t


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("nslots", [64, 192])
def test_pack_windows(layout, nslots):
    for fill in (0, nslots // 2, 7):
        t = crafted_table(layout, nslots, fill, seed=nslots + layout + fill)
        want = t.fps()
        assert len(want) == fill
        for window in (8, 20, 50, nslots, 0):      # many windows (some empty); two that do not divide nslots; whole
            stream, st = pack(layout, t.w, nslots, window)
            assert st[0] == fill and st[3] == fill, (fill, window)
            assert sorted(stream) == want, (fill, window)
            assert len(set(stream)) == fill
            assert (st[1], st[2]) == cm.checksum(want), (fill, window)


@pytest.mark.parametrize("layout", [0, 1])
def test_pack_full_table_and_many_workgroups(layout):
    # every slot occupied (a full window must fit one staging buffer: 512
    # words), and a table of more than one workgroup per window
    r = pm.rng(5)
    n = 512
    fps = [r.getrandbits(63) | 1 for _ in range(n)]
    image = fps if layout else [w for fp in fps for w in (fp, pm.nclaim(2, 9))]
    for window in (0, 512, 100):
        stream, st = pack(layout, image, n, window)
        assert st[0] == n and sorted(stream) == sorted(fps)
        assert (st[1], st[2]) == cm.checksum(fps)
    # 4,096 slots at 1/4 load with a 64-KiB stage: one window of 16 workgroups
    n = 4096
    t = Table(n, KIND[layout])
    fps = [r.getrandbits(63) | 1 for _ in range(n // 4)]
    for fp in fps:
        assert (t.pair_insert(fp) if layout else t.insert(fp)) == pm.CL_NEW
    stream, st = pack(layout, t.w, n, 0, stage=65536)
    assert sorted(stream) == sorted(fps) and (st[1], st[2]) == cm.checksum(fps)


def restore_list(layout, nslots, seed):
    """About 100 fingerprints for `nslots` slots: colliding homes, a run over
    the table's end, the rest anywhere."""
    kind = KIND[layout]
    r = pm.rng(seed)
    last_home = nslots - 2 if layout else nslots - 1
    fps = pm.craft(last_home, nslots, kind, 5, r) + pm.craft(40, nslots, kind, 6, r) + pm.craft(42, nslots, kind, 3, r)
    seen = set(fps)
    while len(fps) < 100:
        fp = r.getrandbits(63) | 1
        if fp not in seen:
            seen.add(fp)
            fps.append(fp)
    r.shuffle(fps)
    return fps


@pytest.mark.parametrize("layout", [0, 1])
def test_restore_matches_the_model(layout):
    nslots = 256
    fps = restore_list(layout, nslots, seed=3 + layout)
    model = Table(nslots, KIND[layout])
    for fp in fps:
        assert (model.pair_insert(fp) if layout else model.insert(fp)) == pm.CL_NEW
    # one fingerprint per launch: the model's sequential inserts, slot for slot
    image, st = restore(layout, fps, nslots, window=1)
    assert st[0] == 0 and (st[1], st[2]) == cm.checksum(fps)
    got = Table(nslots, KIND[layout], image)
    assert [got.fp_at(i) for i in range(nslots)] == [model.fp_at(i) for i in range(nslots)]
    # concurrent launches (all at once; windows of 33 over both staging
    # buffers): the same set in the same occupied slots, every entry on its run
    for window in (0, 33):
        image, st = restore(layout, fps, nslots, window=window)
        assert st[0] == 0 and (st[1], st[2]) == cm.checksum(fps), window
        got = Table(nslots, KIND[layout], image)
        assert got.fps() == model.fps() and got.occupied() == model.occupied(), window
        got.check_runs()
        if layout == 0:
            # restored entries carry level-1 claims: old to every later level
            assert all(((~got.w[2 * i + 1] & pm.M64) >> pm.KEY_BITS) == 1 for i in got.occupied())


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("window", [0, 33])
def test_restore_reports_one_duplicate(layout, window):
    nslots = 256
    fps = restore_list(layout, nslots, seed=9)
    dup = fps[:60] + [fps[10]] + fps[60:]          # (window 33: the copy arrives two launches later)
    image, st = restore(layout, dup, nslots, window=window)
    assert st[0] == 1
    assert Table(nslots, KIND[layout], image).fps() == sorted(fps)


def test_selftest_refuses_bad_arguments():
    lib = kubecheck.load()
    out = np.zeros(8, dtype=np.uint64)
    assert lib.kc_ckpt_selftest(2, 0, 64, _u64(out), 8, 0, 0, _u64(out), _u64(out)) == -22
    assert lib.kc_ckpt_selftest(0, 1, 7, _u64(out), 7, 0, 0, _u64(out), _u64(out)) == -22      # odd compact table
    assert lib.kc_ckpt_selftest(0, 0, 4, _u64(out), 8, 0, 100, _u64(out), _u64(out)) == -22    # stage below 4096
