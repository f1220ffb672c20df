"""The seen-set probe primitives at the table's edges: kc_probe_selftest runs
the product's device functions (fpset_dev.h, lds_claim, the rehash kernels) on
tables of 4-72 slots with fingerprints crafted for a chosen home slot, and the
results and table images are compared with the host model (probe_model.py).
Integers only: every comparison is exact.

Sequential mode (one lane, in order): every result and the whole image equal
the model's.  Concurrent mode (a lane per operation): one winner per
fingerprint, the model's fingerprint set and occupied slots (linear probing
fills the same slots in any order), every fingerprint on its run.

The batch table's loops have no bound, so no case fills one past half (the
harness refuses to); every other loop is bounded by the table's size."""
import ctypes as C

import numpy as np
import pytest

import kubecheck
import probe_model as pm
from probe_model import CL_CUR, CL_FULL, CL_LOST, CL_NEW, CL_OLD, Table

pytestmark = pytest.mark.gpu

SIZES = {"wide": (4, 8, 16, 64, 66), "compact": (4, 8, 16, 64, 66), "fpset": (8, 16, 64, 72)}
LEVEL = 3


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def dev(kind, nslots, fps=(), keys=None, level=LEVEL, mode=0, table=None, n=None, wps=1, nres=None):
    """One kc_probe_selftest call: (result words, table image) as Python ints."""
    lib = kubecheck.load()
    f = np.array(list(fps), dtype=np.uint64)
    k = np.array(list(keys), dtype=np.uint64) if keys is not None else None
    t = np.array(list(table), dtype=np.uint64) if table is not None else None
    n = len(f) if n is None else n
    res = np.zeros(max(1, n if nres is None else nres), dtype=np.uint64)
    out = np.zeros(nslots * wps, dtype=np.uint64)
    kubecheck._lib.check("kc_probe_selftest", lib.kc_probe_selftest(
        kind, nslots, _u64(f) if len(f) else None, _u64(k) if k is not None else None, n, level, mode,
        _u64(t) if t is not None else None, _u64(res), _u64(out)))
    return [int(x) for x in res], [int(x) for x in out]


def signed(x):
    return x - (1 << 64) if x >> 63 else x


# ---- the insert primitives: (table kind, device run, model run); both return
# (results, image) for the operations (fps, keys) on a table image
def _m_each(f):
    def run(kind, n, fps, keys, image):
        t = Table(n, kind, image)
        return [f(t, fp, k) for fp, k in zip(fps, keys)], t.w
    return run


def _m_group(kind, n, fps, keys, image):
    t = Table(n, kind, image)
    res = []
    for i in range(0, len(fps), pm.CLAIM_BATCH):
        res += t.pair_group(fps[i:i + pm.CLAIM_BATCH])
    return res, t.w


def _m_protocol(kind, n, fps, keys, image):
    t = Table(n, kind, image)
    codes, holds = t.store_protocol(fps, keys, LEVEL)
    return codes + holds, t.w


def _d(pk, wps, signed_res=False, double=False):
    def run(kind, n, fps, keys, image, mode=0):
        res, img = dev(pk, n, fps, keys, mode=mode, table=image, wps=wps, nres=2 * len(fps) if double else None)
        return ([signed(r) for r in res] if signed_res else res), img
    return run


INSERTS = {
    "fpset_insert": ("fpset", _d(pm.PK_FPSET_INSERT, 1, signed_res=True), _m_each(lambda t, fp, k: t.fpset_insert(fp))),
    "claimset_claim": ("wide", _d(pm.PK_CLAIM, 2), _m_each(lambda t, fp, k: t.claim(fp, k, LEVEL))),
    "claim_store": ("wide", _d(pm.PK_CLAIM_STORE, 2, double=True), _m_protocol),
    "insert_from": ("wide", _d(pm.PK_INSERT_FROM, 2), _m_each(lambda t, fp, k: t.insert(fp))),
    "insert_pair": ("compact", _d(pm.PK_PAIR, 1), _m_each(lambda t, fp, k: t.pair_insert(fp))),
    "insert_pair_group": ("compact", _d(pm.PK_PAIR_GROUP, 1), _m_group),
}
NEW = {name: 1 if name == "fpset_insert" else CL_NEW for name in INSERTS}
FULL = {name: -1 if name == "fpset_insert" else CL_FULL for name in INSERTS}
PRIMS = sorted(INSERTS)


def both(name, n, fps, keys=None, image=None):
    """Run on the device (sequential) and in the model; assert they agree in
    every result and every table word; return (results, image)."""
    kind, d, m = INSERTS[name]
    keys = list(range(100, 100 + len(fps))) if keys is None else keys
    image = [0] * (n * pm.WORDS[kind]) if image is None else image
    got = d(kind, n, fps, keys, image)
    want = m(kind, n, fps, keys, image)
    assert got[0] == want[0], (name, n)
    assert got[1] == want[1], (name, n)
    return got


def lookups(name, n, fps, image):
    """contains / get of each fp on `image`, device against model."""
    kind = INSERTS[name][0]
    t = Table(n, kind, image)
    if kind == "fpset":
        res, img = dev(pm.PK_FPSET_CONTAINS, n, fps, table=image)
        want = [t.contains(fp) for fp in fps]
    elif kind == "wide":
        res, img = dev(pm.PK_CLAIM_GET, n, fps, table=image, wps=2)
        want = [t.get(fp) for fp in fps]
    else:
        return None
    assert res == want and img == list(image)
    return res


def last_home(kind, n):
    return n - 2 if kind == "compact" else n - 1


def cases(name):
    return [(name, n) for n in SIZES[INSERTS[name][0]]]


ALL = [c for p in PRIMS for c in cases(p)]


@pytest.mark.parametrize("name,n", ALL)
def test_wrap(name, n):
    kind = INSERTS[name][0]
    rng = pm.rng(n * 31 + len(name))
    last = last_home(kind, n)
    # every fingerprint homed at the last slot (pair): the run continues at 0
    m = max(2, min(n - 1, 6))
    fps = pm.craft(last, n, kind, m, rng)
    ops = fps + fps[::-1] + [fps[0]]
    keys = [50 + 7 * ((i * 5) % len(ops)) for i in range(len(ops))]       # later copies with smaller keys too
    res, img = both(name, n, ops, keys)
    t = Table(n, kind, img)
    assert res[:m] == [NEW[name]] * m and NEW[name] not in res[m:2 * m + 1]
    assert t.fp_at(last) == fps[0] and t.fp_at(0) in fps          # it wrapped
    assert t.occupied() == {(last + i) % n for i in range(m)}
    lookups(name, n, fps + pm.craft(last, n, kind, m + 2, rng)[m:], img)
    # homes n-2, n-1, 0, 1 interleaved (the compact table's homes are even)
    homes = [n - 2, 0] if kind == "compact" else [n - 2, n - 1, 0, 1]
    per = max(1, min(3, (n - 1) // len(homes)))
    lists = [pm.craft(h, n, kind, per, rng) for h in homes]
    mix = [l[i] for i in range(per) for l in lists]
    res, img = both(name, n, mix + mix[::2])
    assert res[:len(mix)] == [NEW[name]] * len(mix)
    Table(n, kind, img).check_runs()
    if kind == "fpset":
        # an even home at ns - 2: a whole pair before the wrap (ns - 1 above is
        # the odd home, half a pair first)
        fps = pm.craft(n - 2, n, kind, min(n - 1, 5), rng)
        both(name, n, fps + fps)


@pytest.mark.parametrize("fill", ["full", "one_free"])
@pytest.mark.parametrize("name,n", ALL)
def test_full_table(name, n, fill):
    kind = INSERTS[name][0]
    rng = pm.rng(n * 17 + len(name))
    last = last_home(kind, n)
    nfill = n if fill == "full" else n - 1
    # homes spread so that runs wrap: a third at the last slot, the rest anywhere
    fps = pm.craft(last, n, kind, max(1, nfill // 3), rng)
    while len(fps) < nfill + 3:
        h = rng.randrange(n) & (~1 if kind == "compact" else ~0)
        f = pm.craft(h, n, kind, 1, rng)[0]
        if f not in fps:
            fps.append(f)
    stored, extra = fps[:nfill], fps[nfill:]
    res, img = both(name, n, stored)
    res = res[:nfill]                                    # (claim_store: the codes; the holds flags follow them)
    assert res == [NEW[name]] * nfill and len(Table(n, kind, img).occupied()) == nfill
    # the next distinct ones: table full -> refused and the table unchanged;
    # one free slot -> the first takes it, the second is refused
    res2, img2 = both(name, n, extra[:2], image=img)
    res2 = res2[:2]
    if fill == "full":
        assert res2 == [FULL[name]] * 2 and img2 == img
    elif name == "insert_pair_group":
        # (the group's CASes come first: the second takes the slot when it is in its pair alone)
        assert sorted(res2) == sorted([NEW[name], FULL[name]])
    else:
        assert res2 == [NEW[name], FULL[name]]
    # every present fingerprint is still found at 100 % load, wherever it sits
    res3, img3 = both(name, n, stored[::-1], image=img2)
    res3 = res3[:nfill]
    assert NEW[name] not in res3 and FULL[name] not in res3
    if name not in ("claimset_claim", "claim_store"):
        assert img3 == img2
    # a lookup of an absent fingerprint terminates with 0
    r = lookups(name, n, [extra[2]] + stored, img2)
    if r is not None:
        assert r[0] == 0 and (kind == "wide" or all(r[1:]))


@pytest.mark.parametrize("name,n", ALL)
def test_values(name, n):
    kind = INSERTS[name][0]
    rng = pm.rng(n + 99)
    base = pm.craft(0, n, kind, 1, rng)[0] & ((1 << 59) - 1)
    owners = [base | (o << 59) for o in range(16)][:max(1, n // 2)]       # differ in the top 4 (owner) bits only
    lo = rng.getrandbits(32) | 1
    same_lo = [(h << 32) | lo for h in (1, 2, 0x7fffffff)][:max(1, n // 4)]   # equal low 32 bits
    fps = list(dict.fromkeys([1, (1 << 63) - 1] + owners + same_lo))[:n - 1]
    res, img = both(name, n, fps + fps)
    assert res[:len(fps)] == [NEW[name]] * len(fps)
    assert Table(n, kind, img).fps() == sorted(fps)
    lookups(name, n, fps + [2, (1 << 63) - 2], img)


# ---- the compact table's pair branches, by pre-loading and by a lost CAS
@pytest.mark.parametrize("n", SIZES["compact"])
@pytest.mark.parametrize("where", ["last", "first"])
def test_pair_branches(n, where):
    rng = pm.rng(n + len(where))
    h = n - 2 if where == "last" else 0
    fp, x, y, z = pm.craft(h, n, "compact", 4, rng)
    nxt = (h + 2) % n

    def image(a, b):
        img = [0] * n
        img[h], img[h + 1] = a, b
        return img

    # (pre-loaded pair, expected code, where fp must be afterwards)
    branches = [((0, 0), CL_NEW, h), ((x, 0), CL_NEW, h + 1), ((x, y), CL_NEW, nxt),
                ((fp, 0), CL_OLD, h), ((x, fp), CL_OLD, h + 1)]
    for (a, b), code, at in branches:
        for name in ("insert_pair", "insert_pair_group"):
            res, img = both(name, n, [fp], image=image(a, b))
            assert res == [code] and img[at] == fp, (name, a, b)
    # the pair as a lane loaded it BEFORE the table changed: its CAS into the
    # slot that read empty loses to another fingerprint (or finds fp itself)
    stale = [((0, 0), (x, 0), CL_NEW, h + 1),       # CAS into home lost; home + 1 still empty
             ((0, 0), (x, y), CL_NEW, nxt),         # ... and home + 1 taken meanwhile: past the pair
             ((0, 0), (fp, 0), CL_OLD, h),          # another copy of fp won the CAS
             ((0, 0), (x, fp), CL_OLD, h + 1),      # fp went into home + 1 meanwhile
             ((x, 0), (x, y), CL_NEW, nxt),         # CAS into home + 1 lost
             ((x, 0), (x, fp), CL_OLD, h + 1)]
    if n == 4:
        # both other slots taken as well: the table is full after the lost CAS
        stale.append(((0, 0), (x, y), CL_FULL, None))
    for e, (a, b), code, at in stale:
        img0 = image(a, b)
        if code == CL_FULL:
            img0[nxt], img0[nxt + 1] = z, pm.craft(h, n, "compact", 5, rng)[4]
        res, img = dev(pm.PK_PAIR_STALE, n, [fp], keys=list(e), table=img0)
        t = Table(n, "compact", img0)
        assert res == [t.pair_insert(fp, e)] == [code] and img == t.w, (e, a, b)
        assert at is None or img[at] == fp


# ---- the deterministic protocol on 16-B slots
@pytest.mark.parametrize("n", SIZES["wide"])
def test_store_claim_protocol(n):
    rng = pm.rng(n + 7)
    cnt = min(4, n - 1)
    fps = pm.craft(n - 1, n, "wide", cnt, rng)
    pre = Table(n, "wide")
    old, pend = fps[0], fps[1]
    pre.claim(old, 5, LEVEL - 1)                 # stored by an earlier level
    pre.insert(pend)                             # claim word 0: pending, current level
    img0 = list(pre.w)
    ops = [old, pend, pend] + [f for f in fps[2:] for _ in range(4)]
    keys = [1, 40, 30] + [k for _ in fps[2:] for k in (20, 10, 25, 15)]
    res, img = both("claim_store", n, ops, keys, image=img0)
    codes, holds = res[:len(ops)], res[len(ops):]
    assert codes[:3] == [CL_OLD, CL_CUR, CL_CUR] and holds[:3] == [0, 0, 1]
    t = Table(n, "wide", img)
    assert t.get(old) == pm.nclaim(LEVEL - 1, 5)                  # no write to an old entry
    assert t.get(pend) == pm.nclaim(LEVEL, 30)
    for j, f in enumerate(fps[2:]):
        c = codes[3 + 4 * j: 7 + 4 * j]
        # inserter (20), smaller (10): candidate, 25: a smaller claim is stored, 15: candidate
        assert c == [CL_NEW, CL_CUR, CL_LOST, CL_CUR]
        assert holds[3 + 4 * j: 7 + 4 * j] == [0, 1, 0, 0]        # exactly the minimum holds the slot
        assert t.get(f) == pm.nclaim(LEVEL, 10)
    # claimset_claim on the same pre-loaded table: old / cur / lost without the settle launches
    res, img = both("claimset_claim", n, ops, keys, image=img0)
    assert res[:3] == [CL_OLD, CL_CUR, CL_CUR]


# ---- batch table (never past half full)
@pytest.mark.parametrize("mode", [0, 1])
def test_batch_table(mode):
    rng = pm.rng(11)
    n = 64 if mode == 0 else 8192
    nfp = 10 if mode == 0 else 400
    fps = [rng.getrandbits(63) | 1 for _ in range(nfp - 3)]
    fps += [f for f in (1, (1 << 63) - 1, fps[0] ^ (1 << 62))]
    ops = [rng.choice(fps) for _ in range(n // 2 - nfp)] + fps
    rng.shuffle(ops)
    keys = list(range(7, 7 + len(ops)))
    res, img = dev(pm.PK_BATCH, n, ops, keys, mode=mode, wps=2)
    t = Table(n, "batch")
    want = t.batch(ops, keys)
    assert res == want and sum(res) == nfp
    got = Table(n, "batch", img)
    assert got.occupied() == t.occupied() and got.fps() == t.fps()
    assert all(got.get(f) == t.get(f) for f in fps)
    got.check_runs()
    if mode == 0:
        assert img == t.w
    # a batch table more than half full is refused, not run
    with pytest.raises(kubecheck.KubecheckError):
        dev(pm.PK_BATCH, 8, [1, 2, 3, 4, 5], [0] * 5, wps=2)


# ---- the tile table in LDS
@pytest.mark.parametrize("nt,pk", [(pm.LDS_NT, pm.PK_LDS), (pm.LDS_NT_SH, pm.PK_LDS_SH)])
def test_lds_claim(nt, pk):
    rng = pm.rng(nt)
    # wrap at NT - 1, fingerprints equal in the low 32 bits (same slot, different fp), minimum key
    fps = pm.craft(nt - 1, nt, "lds", 5, rng)
    lo = fps[0] & 0xFFFFFFFF
    fps += [(h << 32) | lo for h in (1, 0x7ffffffe)]
    ops = fps + fps[::-1] + fps[::2]
    keys = [(900 - 37 * i) % 1000 for i in range(len(ops))]
    res, img = dev(pk, nt, ops, keys, wps=2)
    t = Table(nt, "lds")
    want = [t.lds_claim(f, k) for f, k in zip(ops, keys)]
    assert [signed(r) for r in res] == want and img == t.w
    assert t.occupied() == {(nt - 1 + i) % nt for i in range(len(fps))}
    for f in fps:
        assert t.get(f) == min(k for o, k in zip(ops, keys) if o == f)
    # filled to NT (one fingerprint homed in every slot, so the fill is short),
    # one more distinct fingerprint: -1, table unchanged; a stored one: its slot
    fill = [pm.craft(s, nt, "lds", 1, rng)[0] for s in range(nt)]
    extra = pm.craft(nt // 2, nt, "lds", 2, rng)
    extra = [f for f in extra if f not in fill][0]
    ops = fill + [extra, fill[3], fill[nt - 1], extra]
    keys = [5] * nt + [1, 2, 9, 1]
    res, img = dev(pk, nt, ops, keys, wps=2)
    t = Table(nt, "lds")
    want = [t.lds_claim(f, k) for f, k in zip(ops, keys)]
    assert [signed(r) for r in res] == want and img == t.w
    assert want[nt:] == [-1, 3, nt - 1, -1] and t.get(fill[3]) == 2 and t.get(fill[nt - 1]) == 5
    # all but one slot filled through a pre-loaded image, every claim homed at
    # NT - 1: the free slot is found after the wrap, then the table is full
    t = Table(nt, "lds")
    free = 7
    for s in range(nt):
        if s != free:
            t.lds_claim(fill[s], 5)
    more = pm.craft(nt - 1, nt, "lds", 3, rng)
    more = [f for f in more if f not in fill][:2]
    res, img = dev(pk, nt, more + more, [4, 4, 3, 3], table=t.w, wps=2)
    want = [t.lds_claim(f, k) for f, k in zip(more + more, [4, 4, 3, 3])]
    assert [signed(r) for r in res] == want == [free, -1, free, -1] and img == t.w
    # concurrent (256 lanes): the same slots, fingerprints and minimum keys
    distinct = pm.craft(nt - 1, nt, "lds", 40, rng) + pm.craft(0, nt, "lds", 40, rng) + \
        [rng.getrandbits(63) | 1 for _ in range(300)]
    ops = [rng.choice(distinct) for _ in range(3000)] + distinct
    keys = [rng.randrange(1 << 13) for _ in ops]
    res, img = dev(pk, nt, ops, keys, mode=1, wps=2)
    t = Table(nt, "lds")
    for f, k in zip(ops, keys):
        t.lds_claim(f, k)
    got = Table(nt, "lds", img)
    assert got.occupied() == t.occupied() and got.fps() == t.fps()
    got.check_runs()
    for f, r in zip(ops, res):
        assert got.fp_at(r) == f                                   # the slot returned holds fp
    assert all(got.get(f) == t.get(f) for f in distinct)


# ---- rehash kernels: an old table whose runs wrap, into 2x and a non-power-of-two size
@pytest.mark.parametrize("kind,pk,name", [("wide", pm.PK_REHASH_CLAIMSET, "insert_from"),
                                          ("compact", pm.PK_REHASH_FPSLOTS, "insert_pair"),
                                          ("fpset", pm.PK_REHASH_FPSET, "fpset_insert")])
@pytest.mark.parametrize("n", [16, 64])
def test_rehash(kind, pk, name, n):
    rng = pm.rng(n + pk)
    last = last_home(kind, n)
    fps = pm.craft(last, n, kind, n // 4, rng) + pm.craft(0, n, kind, n // 8, rng) + \
        pm.craft(n - 2, n, kind, n // 8, rng)
    fps = list(dict.fromkeys(fps))
    old = Table(n, kind)
    for k, f in enumerate(fps):
        if kind == "wide":
            assert old.claim(f, 1000 + k, LEVEL) == CL_NEW
        else:
            assert old.insert(f) == CL_NEW
    assert old.fp_at(0) and old.fp_at(last)
    for new_n in (2 * n, 3 * n - 8 if kind == "fpset" else 2 * n + 6):
        res, img = dev(pk, new_n, table=old.w, n=n, wps=pm.WORDS[kind], nres=1)
        assert res[0] == 0                                          # fail == 0
        got, want = Table(new_n, kind, img), pm.rehash(old, new_n)
        assert got.fps() == want.fps() == sorted(fps)               # the same multiset
        assert got.occupied() == want.occupied()
        got.check_runs()
        if kind == "wide":
            assert all(got.get(f) == old.get(f) for f in fps)       # claim words travel with their fps
        # every fingerprint is found by the matching primitive
        res, img2 = both(name, new_n, fps, image=img)
        assert res == [0 if kind == "fpset" else CL_OLD] * len(fps) and img2 == img
        r = lookups(name, new_n, fps, img)
        assert r is None or all(r)
    # a new table too small for the entries reports every one that found no slot
    if kind != "fpset":
        res, img = dev(pk, 4, table=old.w, n=n, wps=pm.WORDS[kind], nres=1)
        assert res[0] == len(fps) - 4 and len(Table(4, kind, img).occupied()) == 4


# ---- concurrent mode: a few thousand operations over a few hundred fingerprints
@pytest.mark.parametrize("name", PRIMS)
def test_concurrent(name):
    kind = INSERTS[name][0]
    n = 520 if kind == "fpset" else 514                  # not a power of two
    rng = pm.rng(len(name) * 1000 + n)
    last = last_home(kind, n)
    # clustered at the end and the start (long runs across the boundary), the rest anywhere
    distinct = pm.craft(last, n, kind, 70, rng) + pm.craft(0, n, kind, 40, rng) + pm.craft(n - 2, n, kind, 40, rng)
    while len(distinct) < 400:
        f = rng.getrandbits(63) | 1
        if f not in distinct:
            distinct.append(f)
    distinct = list(dict.fromkeys(distinct))
    ops = [rng.choice(distinct) for _ in range(3600)] + distinct
    rng.shuffle(ops)
    keys = list(range(1, len(ops) + 1))
    rng.shuffle(keys)
    kind_, d, m = INSERTS[name]
    res, img = d(kind, n, ops, keys, [0] * (n * pm.WORDS[kind]), mode=1)
    model = Table(n, kind)
    for f in distinct:
        model.insert(f)
    got = Table(n, kind, img)
    assert 0.5 < len(distinct) / n < 1.0
    assert got.fps() == model.fps()                      # the stored fingerprints
    assert got.occupied() == model.occupied()            # the occupied slots, exactly
    got.check_runs()                                     # each on its run before the first empty slot
    codes = res[:len(ops)]
    by_fp = {}
    for f, k, c in zip(ops, keys, codes):
        by_fp.setdefault(f, []).append((k, c))
    others = {"fpset_insert": {0}, "claimset_claim": {CL_CUR, CL_LOST}, "claim_store": {CL_CUR, CL_LOST}}.get(
        name, {CL_OLD})
    for f, kc in by_fp.items():
        cs = [c for _, c in kc]
        assert cs.count(NEW[name]) == 1, hex(f)
        assert set(cs) - {NEW[name]} <= others, (hex(f), cs)
    if name in ("claimset_claim", "claim_store"):
        for f, kc in by_fp.items():
            assert got.get(f) == pm.nclaim(LEVEL, min(k for k, _ in kc))      # the minimum claim
    if name == "claim_store":
        holds = res[len(ops):]
        for f, k, h in zip(ops, keys, holds):
            assert h == int(k == min(kk for kk, _ in by_fp[f]))              # exactly that operation
