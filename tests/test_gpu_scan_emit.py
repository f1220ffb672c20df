"""The kernels that turn a wide level's newmask words into the next frontier
(csrc/engine_kernels.h), each launched alone by kc_emit_selftest with the
engine's grid and block sizes, on inputs made here: k_tile_scan / k_chunk_scan
and tile_scan_body's marks, k_emit_links, k_emit<M>, k_materialize<M>,
k_parent_chain and spread_tile, for Model<1,1,1> and Model<1,2,1>.  Expected
values come from emit_model.py (plain integers and the host Spec).  Integers
only: every comparison is exact, and every output carries guard elements fore
and aft that must come back untouched."""
import numpy as np
import pytest

import emit_model as em
import kubecheck
from emit_model import FORE, M32, M64

pytestmark = pytest.mark.gpu

U64 = np.uint64
GUARD = 0xA5A5A5A5A5A5A5A5
GUARD32 = 0xA5A5A5A5
GUARD8 = 0xA5
AFT = 8
A_COUNT = 22


def run(kind, par, a=None, b=None, out=None, res=None, cfg=None):
    rc = em.selftest(kind, par, a, b, out, res, cfg)
    assert rc == 0, (rc, kubecheck.load().kc_last_error())


def same(got, want, what):
    """Exact equality of two arrays, naming the first difference."""
    got, want = np.asarray(got, dtype=U64), np.asarray(want, dtype=U64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.nonzero(got != want)[0]
    assert d.size == 0, (what, f"{d.size} differ, first at {int(d[0])}: "
                               f"got {int(got[d[0]]):#x} want {int(want[d[0]]):#x}")


# ------------------------------------------------------------------------ scan
SCAN_T = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 65541]


def scan_values(T, g):
    """The value cases of a scan over T cells; every total stays below 2^32."""
    q = M32 // T
    exact = np.full(T, q, dtype=U64)
    exact[-1] += U64(M32 - q * T)
    one = lambda i, v: np.bincount([i], weights=[v], minlength=T).astype(U64)   # noqa: E731
    return {
        "random": g.integers(0, q + 1, size=T, dtype=U64),
        "zero": np.zeros(T, dtype=U64),
        "only the last cell": one(T - 1, 12345),
        "only cell 0": one(0, 7),
        "all equal": np.full(T, min(q, 3), dtype=U64),
        "total 2^32 - 1": exact,
        "2^32 - 1 in the last cell": np.concatenate([np.zeros(T - 1, dtype=U64), np.array([M32], dtype=U64)]),
    }


def run_scan(tot, reg_ok, chunk, marks=None):
    """One scan launch; checks off (guards, prefix, the cells past T) and returns (off, res)."""
    T = len(tot)
    G4 = 4 * ((T + 3) // 4)
    a = np.concatenate([tot, np.array([0xDEADBEEF, M32, 0x80000001][:G4 - T], dtype=U64)])   # pad cells: garbage
    need = max(G4, T + 1)
    out = np.full(FORE + need + AFT, GUARD32, dtype=U64)
    if marks is None:
        res = np.full(G4, GUARD, dtype=U64)
        run(em.K_SCAN, [T, reg_ok, chunk], a=a, out=out, res=res)
    else:
        res = np.full(17, GUARD, dtype=U64)
        stride, nmark, extra = marks
        run(em.K_MARKS, [T, reg_ok, stride, nmark, M32 if extra is None else extra], a=a, out=out, res=res)
    want = em.exclusive_prefix_np(tot)
    assert int(want[-1]) <= M32
    same(out[:FORE], np.full(FORE, GUARD32, dtype=U64), "fore guard")
    same(out[FORE:FORE + T + 1], want, "off")
    # the cells of the last 16-byte group past T: pad cells read as 0, so they hold the total
    same(out[FORE + T + 1:FORE + need], np.full(need - T - 1, want[-1], dtype=U64), "off past T")
    same(out[FORE + need:], np.full(AFT, GUARD32, dtype=U64), "aft guard")
    if marks is None:
        same(res[T:], a[T:], "pad cells of the input")
        same(res[:T], np.zeros(T, dtype=U64) if chunk else tot, "csum zeroed" if chunk else "tot unchanged")
    return res


@pytest.mark.parametrize("T", SCAN_T)
def test_tile_and_chunk_scan(T):
    g = np.random.default_rng(T)
    for name, tot in scan_values(T, g).items():
        for reg_ok in (0, 1):
            for chunk in (0, 1):
                try:
                    run_scan(tot, reg_ok, chunk)
                except AssertionError as e:
                    raise AssertionError(f"{name}, reg_ok {reg_ok}, chunk {chunk}: {e}") from None


# ----------------------------------------------------------------------- marks
def mark_cases():
    cases = []
    # the owner-major scans of the sharded levels: world rows of T0 (or C) cells, the total at `extra`
    for world in (1, 2, 3, 8, 9, 16):
        for T0 in (1, 3, 5, 64, 261):
            cases.append((world * T0, T0, world, world * T0))
    cases.append((3 * 21846, 21846, 3, 3 * 21846))        # 65,538 cells: past the register path
    cases.append((16 * 4097, 4097, 16, 16 * 4097))
    # {cells, 2, tiles}: the total at mark 1 (k * stride == T), `extra` mid-array
    for cells, tiles in ((8, 4), (8, 8), (9, 1), (1000, 999), (4099, 64), (66000, 4097)):
        cases.append((cells, cells, 2, tiles))
    cases += [
        (12, 4, 4, None),      # k * stride == T exactly at k = 3 < nmark
        (12, 4, 3, None),      # ... at k = 3 == nmark: not a mark
        (13, 4, 4, None), (11, 4, 4, None), (10, 4, 5, None),   # marks past T keep the guard
        (30, 7, 16, 29), (30, 7, 16, 0), (31, 5, 7, 31),        # strides that are no multiple of 4
        (40, 1, 16, 17), (16, 1, 16, 16), (15, 1, 16, 15),      # nmark = 16
        (9, 0, 0, 9), (9, 0, 0, 4), (9, 0, 0, 0), (4100, 0, 0, 4099),   # nmark = 0: only extra
        (9, 3, 3, 10), (9, 3, 3, None), (8, 3, 3, 2000),        # extra past T or absent
        (9, 0, 0, None),                                        # no marks at all
    ]
    return cases


@pytest.mark.parametrize("reg_ok", [0, 1])
def test_scan_marks(reg_ok):
    g = np.random.default_rng(17 + reg_ok)
    for T, stride, nmark, extra in mark_cases():
        tot = g.integers(0, 50000, size=T, dtype=U64)
        res = run_scan(tot, reg_ok, 0, marks=(stride, nmark, extra))
        want = em.marks([int(x) for x in tot], stride, nmark, extra, GUARD32)
        assert [int(x) for x in res] == want, (T, stride, nmark, extra)


# ------------------------------------------------------------------- link emit
LINK_N = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 16640, 16641]
BASE, LEVEL_GIDX, NEXT_GIDX, CHUNK_BASE = (1 << 40) - 3, 0x123456789, 37, 1000


def link_masks(n, g):
    lane63 = np.where(np.arange(n) % 64 == 63, g.integers(1, 1 << 32, size=n, dtype=U64), 0).astype(U64)
    last = np.zeros(n, dtype=U64)
    last[-1] = 0x80010001
    sparse = np.where(g.random(n) < 0.05, U64(1) << g.integers(0, 32, size=n, dtype=U64), 0).astype(U64)
    return {
        "zero": np.zeros(n, dtype=U64),
        "all ones": np.full(n, M32, dtype=U64),          # 2,048 entries per wave: 32 deal rounds
        "only bit 31": np.full(n, 1 << 31, dtype=U64),
        "only the last parent": last,
        "only lane 63": lane63,
        "random sparse": sparse,
        "random dense": g.integers(0, 1 << 32, size=n, dtype=U64),
    }


def link_offsets(masks, mode):
    ttot = np.unpackbits(np.ascontiguousarray(masks, dtype="<u4").view(np.uint8)).reshape(-1, 32).sum(axis=1)
    ttot = np.add.reduceat(ttot, np.arange(0, len(masks), em.TILE)).astype(U64)
    if mode == 0:
        return em.exclusive_prefix_np(ttot)
    csum = np.add.reduceat(ttot, np.arange(0, len(ttot), em.CSUM_TILES))
    return np.concatenate([em.exclusive_prefix_np(csum), ttot])


def run_links(masks, mode, want_link, want_trace, cap, total):
    seclen = FORE + NEXT_GIDX + CHUNK_BASE + total + 1 + AFT
    out = np.full(3 * seclen, GUARD, dtype=U64)
    out[2 * seclen:] = GUARD8
    res = np.full(17, GUARD, dtype=U64)
    run(em.K_LINKS, [len(masks), BASE, LEVEL_GIDX, NEXT_GIDX, cap, CHUNK_BASE, mode, want_link, want_trace, seclen],
        a=masks, b=link_offsets(masks, mode), out=out, res=res)
    o, lw, pw, ow, flags, deg = em.link_emit_np(masks, BASE, LEVEL_GIDX, NEXT_GIDX, cap, CHUNK_BASE)
    want = np.full(3 * seclen, GUARD, dtype=U64)
    want[2 * seclen:] = GUARD8
    o = o.astype(np.int64)
    if want_link:
        want[FORE + o] = lw
    if want_trace:
        want[seclen + FORE + NEXT_GIDX + o] = pw
        want[2 * seclen + FORE + NEXT_GIDX + o] = ow
    same(out[:seclen], want[:seclen], "link")
    same(out[seclen:2 * seclen], want[seclen:2 * seclen], "parent")
    same(out[2 * seclen:], want[2 * seclen:], "ord")
    assert int(res[0]) == flags == (em.DF_CAPACITY if total and cap < CHUNK_BASE + total else 0), "defer_flags"
    assert [int(x) for x in res[1:]] == deg, "outdeg"
    return out[FORE:FORE + total] if want_link and cap >= CHUNK_BASE + total else None


@pytest.mark.parametrize("n", LINK_N)
def test_emit_links(n):
    g = np.random.default_rng(n)
    for k, (name, masks) in enumerate(link_masks(n, g).items()):
        total = int(np.unpackbits(np.ascontiguousarray(masks, dtype="<u4").view(np.uint8)).sum())
        end = CHUNK_BASE + total
        launches = [(mode, wl, wt, end + 1) for mode in (0, 1) for wl, wt in ((1, 0), (0, 1), (1, 1))]
        launches += [((k + j) % 2, 1, 1, cap) for j, cap in enumerate((end, end - 1, max(0, end - 64), 0, 1 << 63))]
        for mode, wl, wt, cap in launches:
            try:
                run_links(masks, mode, wl, wt, cap, total)
            except AssertionError as e:
                raise AssertionError(f"{name}, mode {mode}, link {wl}, trace {wt}, cap {cap - end:+d}: {e}") from None


# -------------------------------------------------------- emit and materialise
# (model, level) -> oracle level index; the widths: Model_1 304 and 3,086, NP=2 3,819
LEVELS = {"narrow": (1, 22), "wide": (1, 41), "np2": (2, 22)}
CUTS = (1, 255, 257, 1025)
_levels = {}


def the_level(name, oracle):
    """(SpecLevel, first-discoverer masks) of an oracle level, computed once."""
    if name not in _levels:
        np_, lv = LEVELS[name]
        cfg = oracle.config(np_=np_)
        tuples, nxt = oracle.level_tuples(cfg, lv), oracle.level_tuples(cfg, lv + 1)
        level = em.SpecLevel(kubecheck.Spec(kubecheck.ModelConfig(np=np_)), tuples)
        new = {t.tobytes() for t in nxt}
        masks = em.first_discoverer_masks(level, set(), new=new)
        assert sum(em.popcount(m) for m in masks) == len(nxt)
        _levels[name] = (level, masks)
    return _levels[name]


def mask_cases(level, first, n):
    full = level.full_masks()[:n]
    return {
        "first discoverer": first[:n],
        "all successors": full,
        "none": [0] * n,
        "last position only": [f & ~(f >> 1) for f in full],
    }


def run_emit(level, masks, mode, keep_trace=1, base=3, next_base=700, chunk_base=1000, level_gidx=5000, next_gidx=41,
             cfg=None):
    """One k_emit launch against the model; returns the new states (total x W words)."""
    n, W = len(masks), level.spec.state_words
    total = sum(em.popcount(m) for m in masks)
    sn = FORE + chunk_base - next_base + total + AFT
    st = FORE + next_gidx + chunk_base + total + AFT
    out = np.full(sn * W + 2 * st, GUARD, dtype=U64)
    out[sn * W + st:] = GUARD8
    res = np.full(2 + A_COUNT + em.OUTDEG_BINS, GUARD, dtype=U64)
    run(em.K_EMIT, [n, base, next_base, chunk_base, level_gidx, next_gidx, keep_trace, mode, sn, st],
        a=level.packed()[:n * W], b=masks, out=out, res=res, cfg=cfg or level.spec.cfg)
    m = em.emit(level, masks, base, next_base, chunk_base, level_gidx, next_gidx, keep_trace)
    want = np.full(sn * W + 2 * st, GUARD, dtype=U64)
    want[sn * W + st:] = GUARD8
    for i, words in m["next"].items():
        want[(FORE + i) * W:(FORE + i + 1) * W] = words
    for i, v in m["parent"].items():
        want[sn * W + FORE + i] = v
    for i, v in m["ord"].items():
        want[sn * W + st + FORE + i] = v
    same(out[:sn * W], want[:sn * W], "next")
    same(out[sn * W:sn * W + st], want[sn * W:sn * W + st], "parent")
    same(out[sn * W + st:], want[sn * W + st:], "ord")
    assert int(res[0]) == m["err_key"], ("err_key", hex(int(res[0])), hex(m["err_key"]))
    assert int(res[1]) == m["next_cand"], "next_cand"
    assert [int(x) for x in res[2:2 + A_COUNT]] == m["act_dist"], "act_dist"
    assert [int(x) for x in res[2 + A_COUNT:]] == m["outdeg"], "outdeg"
    first = (FORE + chunk_base - next_base) * W
    return out[first:first + total * W].copy()


def gpu_links(masks):
    """k_emit_links over the masks with base 0: (link words, trace parents, trace ords) of the new states."""
    n = len(masks)
    total = sum(em.popcount(int(m)) for m in masks)
    seclen = FORE + 7 + total + 1 + AFT
    out = np.full(3 * seclen, GUARD, dtype=U64)
    res = np.zeros(17, dtype=U64)
    m = np.array(masks, dtype=U64)
    run(em.K_LINKS, [n, 0, 9000, 7, total, 0, 0, 1, 1, seclen], a=m, b=link_offsets(m, 0), out=out, res=res)
    assert int(res[0]) == 0
    return (out[FORE:FORE + total], out[seclen + FORE + 7:seclen + FORE + 7 + total],
            out[2 * seclen + FORE + 7:2 * seclen + FORE + 7 + total])


def run_materialize(level, nprev, links, trace, mode, prev_counts, cfg=None):
    """One k_materialize launch against the model; returns the rebuilt states."""
    W = level.spec.state_words
    n = len(links)
    out = np.full((FORE + n + AFT) * W, GUARD, dtype=U64)
    res = np.full(3 + A_COUNT, GUARD, dtype=U64)
    par = [n, nprev, mode, 123 if mode else 0, 9000 if mode else 0, prev_counts]
    b = links if mode == 0 else np.concatenate(trace)
    run(em.K_MATERIALIZE, par, a=level.packed()[:nprev * W], b=b, out=out, res=res, cfg=cfg or level.spec.cfg)
    m = em.materialize(level, em.links_of(links))
    want = np.full((FORE + n + AFT) * W, GUARD, dtype=U64)
    if n:
        want[FORE * W:(FORE + n) * W] = np.concatenate(m["out"])
    same(out, want, "out")
    assert int(res[0]) == m["defer_flags"], "defer_flags"
    assert int(res[1]) == m["defer_inv_n"], ("defer_inv_n", hex(int(res[1])), hex(m["defer_inv_n"]))
    assert int(res[2]) == m["next_cand"], "next_cand"
    assert [int(x) for x in res[3:]] == m["act_dist"], "act_dist"
    return out[FORE * W:(FORE + n) * W].copy()


@pytest.mark.parametrize("name", list(LEVELS))
def test_emit_and_materialize(name, oracle):
    level, first = the_level(name, oracle)
    for n in [c for c in CUTS if c < level.n] + [level.n]:
        for case, masks in mask_cases(level, first, n).items():
            try:
                nxt = run_emit(level, masks, 0)
                same(run_emit(level, masks, 1), nxt, "the two offset modes")
                if case == "first discoverer":
                    same(run_emit(level, masks, 0, keep_trace=0, base=0, next_base=0, chunk_base=0), nxt, "no trace")
                if not any(masks):
                    continue
                # the deferred path's defining property: the links of the link emit, rebuilt, are emit's states
                links, tp, to = gpu_links(masks)
                for mode, pc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    same(run_materialize(level, n, links, (tp, to), mode, pc), nxt, f"materialize {mode} {pc}")
            except AssertionError as e:
                raise AssertionError(f"n {n}, {case}: {e}") from None


def test_emit_and_materialize_report_violations(oracle):
    """variant 2 (an invariant that fails): err_key is the minimum key of the
    level, defer_flags / defer_inv_n name the lowest violating state."""
    ocfg = oracle.config(variant=2)
    ref = oracle.run(ocfg)
    assert ref["err_kind"] == 2
    cfg = kubecheck.ModelConfig(variant=2)
    level = em.SpecLevel(kubecheck.Spec(cfg), oracle.level_tuples(ocfg, ref["err_level"] - 1))
    full = level.full_masks()
    entries = em.new_entries(full)
    bad = [k for k, (i, t) in enumerate(entries) if level.info(i, t)[1]]
    assert bad and level.n > 64
    for mode in (0, 1):
        run_emit(level, full, mode)
        assert em.emit(level, full, base=3)["err_key"] == (3 + entries[bad[0]][0]) << 16 | entries[bad[0]][1] << 8 | 2
    links, tp, to = gpu_links(full)
    for mode, pc in ((0, 0), (1, 1)):
        run_materialize(level, level.n, links, (tp, to), mode, pc)
    assert em.materialize(level, entries)["defer_inv_n"] == ~bad[0] & M64
    # only the last violator, then none: the minimum moves, then nothing is reported
    keep = [0] * level.n
    keep[entries[bad[-1]][0]] = 1 << entries[bad[-1]][1]
    run_emit(level, keep, 0)
    links, tp, to = gpu_links(keep)
    run_materialize(level, level.n, links, (tp, to), 0, 0)
    clean = list(full)
    for k in bad:
        clean[entries[k][0]] &= ~(1 << entries[k][1])
    run_emit(level, clean, 1)
    links, tp, to = gpu_links(clean)
    run_materialize(level, level.n, links, (tp, to), 1, 0)
    # with the invariants off (invariants = 0) the same states raise nothing
    off = kubecheck.ModelConfig(variant=2, invariants=0)
    quiet = em.SpecLevel(kubecheck.Spec(off), level.tuples)
    run_emit(quiet, full, 0)
    run_materialize(quiet, level.n, gpu_links(full)[0], None, 0, 1)


# ---------------------------------------------------------------- parent chain
def chain_arrays(length, g):
    """A chain of `length` states scattered over length + 5 slots; returns (parent, ord, start)."""
    n = length + 5
    order = g.permutation(n)[:length]              # order[0] is the Init state
    parent = np.arange(n, dtype=U64)               # the other slots point at themselves
    ord_ = g.integers(0, 256, size=n, dtype=U64)
    parent[order[0]] = M64
    for k in range(1, length):
        parent[order[k]] = order[k - 1]
    return parent, ord_, int(order[-1])


@pytest.mark.parametrize("cap", [1, 5, 4099])
def test_parent_chain(cap):
    g = np.random.default_rng(cap)
    for length in sorted({1, 2, cap - 1, cap, cap + 1, cap + 7} - {0}):
        parent, ord_, start = chain_arrays(length, g)
        out = np.full(FORE + 1 + cap + AFT, GUARD, dtype=U64)
        run(em.K_CHAIN, [start, cap], a=parent, b=ord_, out=out)
        ln, words = em.parent_chain([int(x) for x in parent], [int(x) for x in ord_], start, cap)
        assert ln == (length if length <= cap else 0)
        want = np.full(FORE + 1 + cap + AFT, GUARD, dtype=U64)
        want[FORE] = ln
        want[FORE + 1:FORE + 1 + len(words)] = words
        same(out, want, f"chain of {length}")          # (cap + 1: len = 0, out[cap] still the guard)


# ---------------------------------------------------------------------- spread
@pytest.mark.parametrize("G", [1, 2, 767, 768, 769, 1536, 1537, 5000])
def test_spread_tile(G):
    for S in (0, 1, 128, 768, 3072):
        out = np.full(FORE + G + AFT, GUARD32, dtype=U64)
        run(em.K_SPREAD, [G, S], out=out)
        tiles = [int(x) for x in out[FORE:FORE + G]]
        assert tiles == [em.spread_tile(b, G, S) for b in range(G)], (G, S)
        assert sorted(tiles) == list(range(G)), (G, S)
        same(np.concatenate([out[:FORE], out[FORE + G:]]), np.full(FORE + AFT, GUARD32, dtype=U64), "guards")
