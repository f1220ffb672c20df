"""The host model of the wide level's scan, emit and rebuild (emit_model.py)
against brute force and hand-worked cases, and on a real level: the masks of
"first discoverer" between two consecutive oracle levels, emitted as links and
rebuilt, give the oracle's next level in order.  Also what kc_emit_selftest
refuses before it looks for a GPU.  No GPU needed."""
import random

import numpy as np
import pytest

import emit_model as em
import kubecheck
from emit_model import M64

U64 = np.uint64
EINVAL, ENODEV = 22, 19


def test_exclusive_prefix():
    assert em.exclusive_prefix([]) == [0]
    assert em.exclusive_prefix([3, 1, 4, 1, 5]) == [0, 3, 4, 8, 9, 14]
    r = random.Random(1)
    for n in (1, 2, 5, 64, 257):
        tot = [r.getrandbits(20) for _ in range(n)]
        off = em.exclusive_prefix(tot)
        assert off == [sum(tot[:t]) for t in range(n + 1)]
        assert [int(x) for x in em.exclusive_prefix_np(tot)] == off
    # a total of exactly 2^32 - 1 stays exact (the numpy variant sums in 64 bits)
    tot = [1 << 31, (1 << 31) - 1, 0]
    assert em.exclusive_prefix(tot)[-1] == em.M32 == int(em.exclusive_prefix_np(tot)[-1])


def test_marks_hand_worked():
    G = 0xA5A5A5A5
    tot = [3, 1, 4, 1, 5]                                  # off = 0 3 4 8 9 | 14
    assert em.marks(tot, 2, 3, 5, G) == [0, 4, 9, 14] + [G] * 13          # extra == T: the total
    assert em.marks(tot, 2, 4, None, G) == [0, 4, 9] + [G] * 14           # 3 * 2 > T: left alone
    assert em.marks(tot, 5, 2, 3, G) == [0, 14, 8] + [G] * 14             # 1 * 5 == T: the total
    assert em.marks(tot, 0, 0, 4, G) == [9] + [G] * 16                    # only extra
    assert em.marks(tot, 1, 16, 6, G) == [0, 3, 4, 8, 9, 14] + [G] * 11   # extra past T: left alone
    # the owner-major shape of the sharded scans: world rows of T cells, mark o = the start of owner o's row
    world, T = 3, 4
    cells = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    m = em.marks(cells, T, world, world * T, G)
    assert m[:4] == [0, 10, 36, 78] and m[4:] == [G] * 13


def test_link_emit_hand_worked():
    masks = [0b101, 0, 0x80000000]
    link, parent, ord_, flags, deg = em.link_emit(masks, 10, 100, 7, 1 << 40, 1000)
    assert link == {1000: 10 << 8 | 0, 1001: 10 << 8 | 2, 1002: 12 << 8 | 31}
    assert parent == {1007: 110, 1008: 110, 1009: 112} and ord_ == {1007: 0, 1008: 2, 1009: 31}
    assert flags == 0 and deg == [1, 1, 1] + [0] * 13
    # the entry at cap is dropped, the one before it kept
    link, parent, ord_, flags, _ = em.link_emit(masks, 10, 100, 7, 1002, 1000)
    assert sorted(link) == [1000, 1001] and sorted(parent) == [1007, 1008] and flags == em.DF_CAPACITY
    assert em.link_emit(masks, 10, 100, 7, 1003, 1000)[3] == 0
    assert em.link_emit(masks, 10, 100, 7, 0, 1000)[:4] == ({}, {}, {}, em.DF_CAPACITY)
    assert em.link_emit([0, 0], 0, 0, 0, 0, 0)[3] == 0                    # nothing to drop
    # the last outdegree bin takes 15 and more
    assert em.outdeg_hist([0x7fff, 0xffff, 0xffffffff, 0x3fff]) == [0] * 14 + [1, 3]


def test_link_emit_numpy_agrees():
    r = random.Random(2)
    for n in (1, 63, 257, 700):
        for dense in (0, 1, 2):
            masks = [r.getrandbits(32) & (M64 if dense == 2 else r.getrandbits(32) if dense else
                                          (1 << r.randrange(32)) * (r.random() < 0.2)) for _ in range(n)]
            total = sum(em.popcount(m) for m in masks)
            for cap in (1 << 50, 5 + total, 5 + total - 1, 5 + max(0, total - 64), 0):
                link, parent, ord_, flags, deg = em.link_emit(masks, 1 << 40, 12345, 9, cap, 5)
                o, lw, pw, ow, nflags, ndeg = em.link_emit_np(masks, 1 << 40, 12345, 9, cap, 5)
                assert {int(k): int(v) for k, v in zip(o, lw)} == link
                assert {int(k) + 9: int(v) for k, v in zip(o, pw)} == parent
                assert {int(k) + 9: int(v) for k, v in zip(o, ow)} == ord_
                assert (nflags, ndeg) == (flags, deg)
    assert em.new_entries([0b1010, 0, 1]) == [(0, 1), (0, 3), (2, 0)]


def test_chunk_offsets():
    ttot = list(range(1, 131))                              # 130 tiles: chunks of 64, 64 and 2
    assert em.chunk_offsets(ttot) == [0, sum(ttot[:64]), sum(ttot[:128]), sum(ttot)]
    assert em.tile_counts([1] * 256 + [3] * 2) == [256, 4]


def test_parent_chain():
    NONE = M64
    parent, ord_ = [NONE, 0, 1, 1, 3], [9, 8, 7, 6, 5]
    assert em.parent_chain(parent, ord_, 0, 4) == (1, [9])
    assert em.parent_chain(parent, ord_, 2, 4) == (3, [2 << 8 | 7, 1 << 8 | 8, 9])
    assert em.parent_chain(parent, ord_, 4, 4) == (4, [4 << 8 | 5, 3 << 8 | 6, 1 << 8 | 8, 9])
    assert em.parent_chain(parent, ord_, 4, 3) == (0, [4 << 8 | 5, 3 << 8 | 6, 1 << 8 | 8])   # longer than cap
    assert em.parent_chain([0], [1], 0, 5) == (0, [1] * 5)                                       # a cycle
    assert em.parent_chain(parent, ord_, 0, 0) == (0, [])


@pytest.mark.parametrize("G", [1, 2, 3, 5, 7, 64, 767, 768, 769, 1536, 1537, 5000])
def test_spread_is_a_bijection(G):
    for S in (0, 1, 2, 3, 128, 768, 3072):
        tiles = [em.spread_tile(b, G, S) for b in range(G)]
        assert sorted(tiles) == list(range(G)), (G, S)
        if 0 < S < G:
            # column x = the blocks b = x, x + S, ...: consecutive tiles, the columns in tile order
            cols = [tiles[x::S] for x in range(S)]
            assert all(c == list(range(c[0], c[0] + len(c))) for c in cols)
            assert [t for c in cols for t in c] == list(range(G))
        else:
            assert tiles == list(range(G))
    assert [em.spread_tile(b, 5, 2) for b in range(5)] == [0, 3, 1, 4, 2]


# ------------------------------------------------------------------ a real level
LEVEL = 30


@pytest.fixture(scope="module")
def real_level(oracle):
    cfg = oracle.config()
    spec = kubecheck.Spec(kubecheck.ModelConfig())
    seen = set()
    for lv in range(LEVEL + 1):
        tuples = oracle.level_tuples(cfg, lv)
        seen.update(t.tobytes() for t in tuples)
    level = em.SpecLevel(spec, tuples)
    return spec, level, em.first_discoverer_masks(level, seen), oracle.level_tuples(cfg, LEVEL + 1)


def test_first_discoverer_round_trip(real_level):
    spec, level, masks, nxt = real_level
    assert level.n > 256 and any(masks) and masks != level.full_masks()
    want = [[int(w) for w in spec.pack(t)] for t in nxt]
    # links, then the rebuild
    link, parent, ord_, flags, deg = em.link_emit(masks, 0, 1000, 1000 + level.n, 1 << 40, 0)
    assert sorted(link) == list(range(len(nxt))) and flags == 0
    assert sum(k * v for k, v in enumerate(deg)) == len(nxt) and sum(deg) == level.n
    mat = em.materialize(level, em.links_of([link[o] for o in range(len(nxt))]))
    assert [[int(w) for w in s] for s in mat["out"]] == want
    assert (mat["defer_flags"], mat["defer_inv_n"]) == (0, 0)
    # the same from the trace entries
    first = 1000 + level.n
    pairs = [(parent[first + o] - 1000, ord_[first + o]) for o in range(len(nxt))]
    assert pairs == em.links_of([link[o] for o in range(len(nxt))])
    # the materialising emit agrees with the rebuild
    e = em.emit(level, masks, next_gidx=first, level_gidx=1000)
    assert [[int(w) for w in e["next"][o]] for o in range(len(nxt))] == want
    assert e["err_key"] == M64 and e["act_dist"] == mat["act_dist"] and e["next_cand"] == mat["next_cand"]
    assert (e["parent"], e["ord"]) == (parent, ord_)
    assert sum(e["act_dist"]) == len(nxt)


def test_error_key_and_defer_inv_n(oracle):
    """variant 2 (Force adds without replacing): the level before the oracle's
    error holds a parent with a violating successor; the minimum key names the
    first one in (parent, position) order, the rebuild the lowest index."""
    ref = oracle.run(oracle.config(variant=2))
    assert ref["err_kind"] == 2
    spec = kubecheck.Spec(kubecheck.ModelConfig(variant=2))
    level = em.SpecLevel(spec, oracle.level_tuples(oracle.config(variant=2), ref["err_level"] - 1))
    masks = level.full_masks()
    bad = [(i, t) for i, t in em.new_entries(masks) if level.info(i, t)[1]]
    assert bad
    e = em.emit(level, masks, base=5)
    assert e["err_key"] == (5 + bad[0][0]) << 16 | bad[0][1] << 8 | 2
    mat = em.materialize(level, em.new_entries(masks))
    assert mat["defer_flags"] == em.DF_INVARIANT
    assert mat["defer_inv_n"] == ~em.new_entries(masks).index(bad[0]) & M64
    # with no invariant checked nothing is reported
    quiet = em.SpecLevel(kubecheck.Spec(kubecheck.ModelConfig(variant=2, invariants=0)), level.tuples)
    assert em.emit(quiet, masks)["err_key"] == M64 and em.materialize(quiet, bad)["defer_flags"] == 0


# ------------------------------------------------- what the harness refuses
def _refused(kind, par, a=None, b=None, nout=64, nres=64, cfg=None):
    out, res = np.zeros(nout, dtype=U64), np.zeros(nres, dtype=U64)
    rc = em.selftest(kind, par, a, b, out, res, cfg)
    assert rc in (-EINVAL, -ENODEV, 0), rc
    return rc == -EINVAL


def test_harness_refuses_bad_input(real_level):
    spec, level, masks, nxt = real_level
    F = em.FORE
    assert em.selftest(7, [1]) == -EINVAL and em.selftest(-1, [1]) == -EINVAL
    assert b"kc_emit_selftest" in kubecheck.load().kc_last_error()
    # scan: a without the pad cells, off one cell short (T + 1 and 4 * ceil(T / 4)), a total of 2^32, 17 marks
    assert _refused(em.K_SCAN, [5, 1, 0], a=[1] * 5, nres=5)
    assert _refused(em.K_SCAN, [4, 1, 0], a=[1] * 4, nout=F + 4, nres=4)
    assert _refused(em.K_SCAN, [5, 1, 0], a=[1] * 8, nout=F + 7, nres=8)
    assert _refused(em.K_SCAN, [2, 1, 0], a=[1 << 31, 1 << 31, 0, 0], nres=4)
    assert _refused(em.K_SCAN, [2, 2, 0], a=[1, 1, 0, 0], nres=4)
    assert _refused(em.K_MARKS, [4, 1, 1, 17, 0], a=[1] * 4, nres=17)
    assert not _refused(em.K_SCAN, [5, 1, 0], a=[1] * 8, nout=F + 8, nres=8)
    assert not _refused(em.K_MARKS, [4, 1, 1, 16, 4], a=[1] * 4, nres=17)
    # link emit: wrong offsets, a section that could not take every entry and one more
    m3, sec = [0b11, 0, 0b1], F + 2 + 3 + 3 + 1
    par = [3, 0, 0, 2, 99, 3, 0, 1, 1, sec]
    assert not _refused(em.K_LINKS, par, a=m3, b=[0, 3], nout=3 * sec, nres=17)
    assert _refused(em.K_LINKS, par, a=m3, b=[0, 2], nout=3 * sec, nres=17)
    assert _refused(em.K_LINKS, par, a=m3, b=[1, 3], nout=3 * sec, nres=17)
    assert _refused(em.K_LINKS, par[:9] + [sec - 1], a=m3, b=[0, 3], nout=3 * (sec - 1), nres=17)
    assert _refused(em.K_LINKS, par, a=m3 + [1 << 32], b=[0, 3], nout=3 * sec, nres=17)
    parc = par[:6] + [1] + par[7:]
    assert not _refused(em.K_LINKS, parc, a=m3, b=[0, 3, 3], nout=3 * sec, nres=17)
    assert _refused(em.K_LINKS, parc, a=m3, b=[0, 3, 2], nout=3 * sec, nres=17)
    # emit: a mask bit at the successor count, a word that is no state, next_base past chunk_base, a short section
    n, W = 3, spec.state_words
    pk, full = level.packed()[:n * W], level.full_masks()[:n]
    tot = sum(em.popcount(m) for m in full)
    par = [n, 0, 0, 0, 0, 0, 1, 0, F + tot, F + tot]
    size = (F + tot) * W + 2 * (F + tot)
    assert not _refused(em.K_EMIT, par, a=pk, b=full, nout=size, nres=40)
    assert _refused(em.K_EMIT, par, a=pk, b=[full[0] << 1 | 1] + full[1:], nout=size + W + 2, nres=40)
    assert _refused(em.K_EMIT, par, a=[M64] * (n * W), b=full, nout=size, nres=40)
    assert _refused(em.K_EMIT, [n, 0, 1, 0] + par[4:], a=pk, b=full, nout=size, nres=40)
    assert _refused(em.K_EMIT, par[:8] + [F + tot - 1, F + tot], a=pk, b=full, nout=size - W, nres=40)
    assert _refused(em.K_EMIT, par, a=pk, b=full, nout=size, nres=40, cfg=kubecheck.ModelConfig(np=3))
    # materialise: a parent outside the previous frontier, a position at the successor count
    ok = [(0 << 8) | 0, (2 << 8) | (em.popcount(full[2]) - 1)]
    mp = [2, n, 0, 0, 0, 0]
    assert not _refused(em.K_MATERIALIZE, mp, a=pk, b=ok, nout=(F + 2) * W, nres=25)
    assert _refused(em.K_MATERIALIZE, mp, a=pk, b=[ok[0], n << 8], nout=(F + 2) * W, nres=25)
    assert _refused(em.K_MATERIALIZE, mp, a=pk, b=[ok[0], ok[1] + 1], nout=(F + 2) * W, nres=25)
    assert _refused(em.K_MATERIALIZE, mp, a=pk, b=ok, nout=(F + 1) * W, nres=25)
    assert _refused(em.K_MATERIALIZE, [2, n, 1, 4, 100, 0], a=pk, b=[100, 99, 0, 0], nout=(F + 2) * W, nres=25)
    assert not _refused(em.K_MATERIALIZE, [2, n, 1, 4, 100, 1], a=pk, b=[100, 102, 0, 0], nout=(F + 2) * W, nres=25)
    # parent chain: an entry outside the array, g outside, out shorter than fore + 1 + cap; spread: G of 0
    assert _refused(em.K_CHAIN, [0, 4], a=[M64, 2], b=[0, 0], nout=F + 5)
    assert _refused(em.K_CHAIN, [2, 4], a=[M64, 0], b=[0, 0], nout=F + 5)
    assert _refused(em.K_CHAIN, [1, 4], a=[M64, 0], b=[0, 0], nout=F + 4)
    assert not _refused(em.K_CHAIN, [1, 4], a=[M64, 0], b=[0, 0], nout=F + 5)
    assert _refused(em.K_SPREAD, [0, 1]) and _refused(em.K_SPREAD, [57, 1]) and not _refused(em.K_SPREAD, [56, 1])
