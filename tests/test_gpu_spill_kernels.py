"""The kernels that join the seen-set's two tiers (csrc/engine_spill.h), each
launched alone by kc_spill_selftest as the engine launches it, on tables,
parents and masks made here: k_claimset_keys (the flush), k_spill_queries<M>
(winners -> cold keys), k_spill_apply with claimset_retire (cold hits lose)
and k_tile_succ<M>, for Model<1,1,1> and Model<1,2,1>.  Expected values come
from the host Spec (successors, fingerprints), cold_model.cold_key and the
table model of probe_model.py.  Integers only: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import cold_model as cm
import kubecheck
import probe_model as pm
from cold_model import M64, cold_key

pytestmark = pytest.mark.gpu

U64 = np.uint64
GUARD = 0xA5A5A5A5A5A5A5A5
GUARD32 = 0xA5A5A5A5
RETIRED = M64
K_KEYS, K_QUERIES, K_APPLY, K_TILE = range(4)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None


def spill(kind, np_=1, a=None, b=None, c=None, cap=0, out=None, res=None, nb=None, want=0):
    a, b, c = (None if x is None else np.ascontiguousarray(x, dtype=U64) for x in (a, b, c))
    rc = kubecheck.load().kc_spill_selftest(
        kind, np_, _p(a), 0 if a is None else (len(a) // 2 if kind in (K_KEYS, K_APPLY) else na_states(a, np_)),
        _p(b), (0 if b is None else len(b)) if nb is None else nb, _p(c), 0 if c is None else len(c), cap,
        _p(out), 0 if out is None else len(out), _p(res))
    assert rc == want, kubecheck.load().kc_last_error()
    return rc


def state_words(np_):
    return kubecheck.Spec(kubecheck.ModelConfig(np=np_)).state_words


def na_states(a, np_):
    return len(a) // state_words(np_)


# ------------------------------------------------------------------ k_claimset_keys
def table_image(nslots, live, retired):
    """{slot: fp} for live and retired slots -> image words."""
    img = np.zeros(2 * nslots, dtype=U64)
    for s, fp in live.items():
        img[2 * s], img[2 * s + 1] = fp, pm.nclaim(3, s & 0xffff) if s % 3 else 0     # (0: a pending claim is live)
    for s, fp in retired.items():
        img[2 * s], img[2 * s + 1] = fp, RETIRED
    return img


def claimset_keys(img, cap, nout):
    out = np.full(nout, GUARD, dtype=U64)
    res = np.zeros(1, dtype=U64)
    spill(K_KEYS, a=img, cap=cap, out=out, res=res)
    return [int(x) for x in out], int(res[0])


def fps_for(slots, r):
    fps = {}
    for s in slots:
        fps[s] = r.getrandbits(63) | 1
    return fps


@pytest.mark.parametrize("nslots", [2, 8, 63, 64, 65, 255, 257])
def test_claimset_keys(nslots):
    r = cm.rng(nslots)
    every = list(range(nslots))
    cases = {
        "empty": ([], []),
        "full": (every, []),
        "all retired": ([], every),
        "mixed": (every[::3], every[1::3]),
        "last slot": ([nslots - 1], every[:nslots - 1:2]),
        "last wave": (every[nslots - 1 - (nslots - 1) % 64:], every[:nslots - 1 - (nslots - 1) % 64:2]),
    }
    for name, (live, retired) in cases.items():
        lf, rf = fps_for(live, r), fps_for(retired, r)
        img = table_image(nslots, lf, rf)
        want = sorted(cold_key(fp) for fp in lf.values())
        out, count = claimset_keys(img, nslots, nslots + 8)
        assert count == len(want), name
        assert sorted(out[:count]) == want, name
        assert out[count:] == [GUARD] * (nslots + 8 - count), name
        # a cap below the live count: the count is still the total, cap words are written, the rest keep the pattern
        for cap in {0, 1, len(want) // 2, max(0, len(want) - 1)}:
            if cap >= len(want):
                continue
            out, count = claimset_keys(img, cap, nslots + 8)
            assert count == len(want), (name, cap)
            assert len(set(out[:cap])) == cap and set(out[:cap]) <= set(want), (name, cap)
            assert out[cap:] == [GUARD] * (nslots + 8 - cap), (name, cap)


def test_claimset_keys_grid_stride():
    # more slots than one pass of table_grid's 65,536 workgroups covers
    nslots = (1 << 24) + 300
    r = cm.rng(99)
    live = sorted({0, 63, 64, (1 << 24) - 1, 1 << 24, (1 << 24) + 255, (1 << 24) + 256, nslots - 1} |
                  {r.randrange(nslots) for _ in range(3000)})
    retired = sorted({r.randrange(nslots) for _ in range(3000)} - set(live))
    g = np.random.default_rng(3)
    img = np.zeros(2 * nslots, dtype=U64)
    lf = g.integers(1, 1 << 63, size=len(live), dtype=U64)
    img[2 * np.array(live)] = lf
    img[2 * np.array(live) + 1] = U64(pm.nclaim(3, 5))
    img[2 * np.array(retired)] = g.integers(1, 1 << 63, size=len(retired), dtype=U64)
    img[2 * np.array(retired) + 1] = U64(RETIRED)
    out, count = claimset_keys(img, len(live) + 8, len(live) + 16)
    assert count == len(live)
    assert sorted(out[:count]) == sorted(cold_key(int(fp)) for fp in lf)
    assert out[count:] == [GUARD] * 16


# ------------------------------------------------------------------ parents of the two models
NS = (1, 63, 64, 65, 255, 256, 257, 600)
LEVEL = {1: 40, 2: 30}
_parents = {}


def parents(np_, oracle):
    """600 parents of one level: (packed words, per parent the successors'
    cold keys in position order), computed once per model."""
    if np_ not in _parents:
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=np_))
        tuples = oracle.level_tuples(oracle.config(np_=np_), LEVEL[np_])[:600]
        assert len(tuples) == 600
        packed = np.concatenate([spec.pack(t) for t in tuples])
        keys = []
        for t in tuples:
            succ, fail = spec.successors(t)
            assert fail is None and len(succ) <= 32
            keys.append([cold_key(spec.fingerprint(s)) for _, s in succ])
        # some wave of 64 parents has more than 64 successors: the dealing loop's second round
        assert max(sum(len(k) for k in keys[w:w + 64]) for w in range(0, 600, 64)) > 64
        _parents[np_] = (packed, keys)
    return _parents[np_]


def masks(keys, n, r):
    """newmask words of the first n parents by case name."""
    full = [(1 << len(k)) - 1 for k in keys[:n]]
    out = {"clear": [0] * n, "all": full}
    for k in range(3):
        out[f"random {k}"] = [f & r.getrandbits(32) for f in full]
    wave = (n - 1) // 64 * 64 if n > 64 else 0
    heavy = max(range(wave, min(n, wave + 64)), key=lambda i: len(keys[i]))
    out["one heavy lane"] = [full[i] if i == heavy else 0 for i in range(n)]
    out["only the last parent"] = [0] * (n - 1) + [full[n - 1]]
    return out


@pytest.mark.parametrize("np_", [1, 2])
def test_spill_queries(np_, oracle):
    packed, keys = parents(np_, oracle)
    sw = state_words(np_)
    r = cm.rng(np_)
    for n in NS:
        for name, mask in masks(keys, n, r).items():
            want_k, want_l, tile_off = [], [], []
            for i, m in enumerate(mask):
                if i % 256 == 0:
                    tile_off.append(len(want_k))
                for t in range(32):
                    if (m >> t) & 1:
                        want_k.append(keys[i][t])
                        want_l.append(i << 5 | t)
            nout = len(want_k) + 8
            qkey, qloc = np.full(nout, GUARD, dtype=U64), np.full(nout, GUARD32, dtype=U64)
            spill(K_QUERIES, np_, a=packed[:n * sw], b=mask, c=tile_off, out=qkey, res=qloc)
            assert [int(x) for x in qkey] == want_k + [GUARD] * 8, (n, name)
            assert [int(x) for x in qloc] == want_l + [GUARD32] * 8, (n, name)
    # the harness keeps the kernel inside its buffers: a bit past the successor count, a wrong offset
    n = 65
    full = [(1 << len(k)) - 1 for k in keys[:n]]
    out = np.full(4096, GUARD, dtype=U64)
    spill(K_QUERIES, np_, a=packed[:n * sw], b=[full[0] << 1] + full[1:], c=[0], out=out, res=out.copy(), want=-22)
    spill(K_QUERIES, np_, a=packed[:n * sw], b=full, c=[1], out=out, res=out.copy(), want=-22)
    spill(K_QUERIES, np_, a=packed[:n * sw], b=full, c=[0], out=out[:8], res=out[:8].copy(), want=-22)


@pytest.mark.parametrize("np_", [1, 2])
def test_tile_succ(np_, oracle):
    packed, keys = parents(np_, oracle)
    sw = state_words(np_)
    for n in NS:
        tiles = -(-n // 256)
        res = np.full(tiles, GUARD, dtype=U64)
        spill(K_TILE, np_, a=packed[:n * sw], res=res)
        assert [int(x) for x in res] == [sum(len(k) for k in keys[t * 256:min(n, t * 256 + 256)]) for t in range(tiles)]


# ------------------------------------------------------------------ k_spill_apply, claimset_retire
def apply_model(table, queries, newmask):
    """(overflow, newmask, tile_total) after k_spill_apply; `table` is changed."""
    newmask = list(newmask)
    tiles = -(-len(newmask) // 256)
    total = [sum(bin(m).count("1") for m in newmask[t * 256:t * 256 + 256]) for t in range(tiles)]
    overflow = 0
    for key, loc, found in queries:
        if not found:
            continue
        newmask[loc >> 5] &= ~(1 << (loc & 31))
        total[loc >> 13] -= 1
        i, there = table.locate(cm.cold_unkey(key))
        if there:
            table.w[2 * i + 1] = RETIRED
        else:
            overflow += 1
    return overflow, newmask, total


def run_apply(table, queries, newmask):
    n = table.n
    img = np.array(table.w, dtype=U64)
    out = np.zeros(2 * n, dtype=U64)
    tiles = -(-len(newmask) // 256)
    res = np.zeros(1 + len(newmask) + tiles, dtype=U64)
    flat = [x for q in queries for x in q]
    spill(K_APPLY, a=img, b=flat, nb=len(queries), c=newmask, cap=len(newmask), out=out, res=res)
    want = apply_model(table, queries, newmask)
    res = [int(x) for x in res]
    assert res[0] == want[0]
    assert res[1:1 + len(newmask)] == want[1]
    assert res[1 + len(newmask):] == want[2]
    assert [int(x) for x in out] == table.w
    # only claim words changed, and only to "retired"
    assert [int(x) for x in out[0::2]] == [int(x) for x in img[0::2]]
    assert all(int(a) == int(b) or int(a) == RETIRED for a, b in zip(out[1::2], img[1::2]))
    return res


@pytest.mark.parametrize("nslots", [8, 64, 66])
def test_spill_apply(nslots):
    r = cm.rng(nslots + 1)
    NPAR = 600
    # a run homed at the last slot that wraps (slots n-1, 0, 1), and a few others: the table stays half empty
    wrap = pm.craft(nslots - 1, nslots, "wide", 3, r)
    others = [pm.craft(s, nslots, "wide", 1, r)[0] for s in ([3] if nslots == 8 else [5, 5, 17, 30, 31, nslots - 3])]
    fps = wrap + others

    def fresh():
        t = pm.Table(nslots, "wide")
        for k, fp in enumerate(fps):
            assert t.claim(fp, 100 + k, 3) == pm.CL_NEW
        assert t.locate(wrap[2]) == (1, True)
        return t

    # each fingerprint a winner at its own place: two share a newmask word, two more a tile, one sits in tile 2
    locs = [(7, 0), (7, 5), (200, 31), (300, 2), (599, 1), (256, 0), (255, 9), (1, 1), (2, 2)][:len(fps)]
    base = [r.getrandbits(32) for _ in range(NPAR)]
    for p, t in locs:
        base[p] |= 1 << t
    for name, found in {"none": [0] * len(fps), "all": [1] * len(fps), "the wrapped one": [0, 0, 1] + [0] * (len(fps) - 3),
                        "mixed": [k % 2 for k in range(len(fps))], "same word": [1, 1] + [0] * (len(fps) - 2)}.items():
        q = sorted((cold_key(fp), p << 5 | t, f) for fp, (p, t), f in zip(fps, locs, found))
        t = fresh()
        res = run_apply(t, q, base)
        assert res[0] == 0, name
        assert sum(1 for i in range(nslots) if t.w[2 * i + 1] == RETIRED) == sum(found), name
    # a found key whose fingerprint is not in the table (the protocol never produces one): counted, table unchanged;
    # its run ends at an empty slot (the table is not full)
    t = fresh()
    absent = [pm.craft(nslots - 1, nslots, "wide", 4, r)[3], pm.craft(4 if nslots > 8 else 5, nslots, "wide", 1, r)[0]]
    assert not any(t.locate(fp)[1] for fp in absent)
    q = sorted([(cold_key(fp), p << 5 | t_, 1) for fp, (p, t_) in zip(fps, locs)][:2] +
               [(cold_key(fp), p << 5 | t_, 1) for fp, (p, t_) in zip(absent, [(10, 3), (400, 4)])])
    for _, loc, _ in q:
        base[loc >> 5] |= 1 << (loc & 31)
    before = list(t.w)
    res = run_apply(t, q, base)
    assert res[0] == 2
    assert [a != b for a, b in zip(before, t.w)].count(True) == 2
    # the harness refuses a found query whose newmask bit is clear, and a place outside the parents
    img = np.array(t.w, dtype=U64)
    out, rs = np.zeros(2 * nslots, dtype=U64), np.zeros(1 + 4 + 1, dtype=U64)
    spill(K_APPLY, a=img, b=[5, 1 << 5 | 3, 1], nb=1, c=[0, 0, 0, 0], cap=4, out=out, res=rs, want=-22)
    spill(K_APPLY, a=img, b=[5, 4 << 5 | 3, 0], nb=1, c=[0, 0, 0, 0], cap=4, out=out, res=rs, want=-22)
