"""k_claim and the settle passes (csrc/engine_kernels.h), one launch set per
case through kc_claim_selftest, on frontiers and seen-set images made here,
against claim_model.py (plain Python over kubecheck.Spec).  Integers only:
every comparison is equality or a set relation, every output section carries
guards fore and aft that must come back untouched (claim_model.selftest), and
every case asserts the model's own preconditions ("this tile has more than 256
representatives", "this block has 2,048 distinct successors") before it
touches the device.

Reached per kind (0 exact + settle, 1 / 2 first-claim on 16-B slots / the
compact table, 3 sharded + staging): partial and several tiles, chunk starts,
every spread_tile branch, pre-loaded old and same-level claims, the candidate
overflow list and k_settle_ovf<1>, the LDS table exactly full (kinds 0-2) and
overflowing (kind 3: the lds_claim < 0 branch), chunk sums over 65 and 129
tiles, the deferred rebuild, Assert / deadlock / invariant reports, record
staging at world 2, 3, 4, 8 and a staging buffer that is too small.
Not reached: the engine's own LDS-overflow branch (no state with 9 distinct
successors exists in NP=3 levels 21 and 24, enumerated whole), ocsum as
k_claim adds into it, the sharded deferred rebuild inside k_claim, a full
seen-set (CL_FULL).  TLC-order claim keys, the received records' passes of
k_settle_both, the rebuild through k_shard_materialize and k_owner_cscan on
made chunk sums are test_gpu_shard_kernels.py's."""
import numpy as np
import pytest

import claim_model as cm
import kubecheck
from claim_model import K_EXACT, K_FIRST, K_FIRST_C8, K_SHARD, M64, TILE

pytestmark = pytest.mark.gpu

U64 = np.uint64
LEVEL = 9                      # the successors' level in every case
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def np2_level(oracle):
    """NP=2 level 22 (3,819 parents) as a Frontier, computed once."""
    def make():
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=2))
        return cm.Frontier(spec, oracle.level_tuples(oracle.config(np_=2), 22))
    return cached("np2", make)


def take(fr, index):
    """A frontier over the same block of distinct parents (the successor lists are shared)."""
    sub = cm.Frontier.__new__(cm.Frontier)
    sub.spec, sub.block, sub.index = fr.spec, fr.block, [fr.index[k] for k in index]
    sub.n, sub.tiles = len(sub.index), (len(sub.index) + TILE - 1) // TILE
    return sub


def full_block(oracle):
    """256 pairwise successor-disjoint parents of NP=3 level 21 with 8 distinct
    successors each: 2,048 distinct fingerprints, the engine's LDS table exactly
    full.  Greedy over the level in BFS order (under a second).  No state of
    levels 21 and 24 has 9 distinct successors (both enumerated whole here and
    when this test was written), so there is no 2,049-fingerprint case."""
    def make():
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=3))
        used, block, most = set(), [], 0
        for x in oracle.level_tuples(oracle.config(np_=3), 21):
            s, fail = spec.successors(x)
            if fail is not None:
                continue
            keys = {y.tobytes() for _, y in s}
            most = max(most, len(keys))
            if len(keys) == 8 and not (keys & used) and len(block) < 256:
                used |= keys
                block.append(x)
        assert most == 8 and len(block) == 256
        fr = cm.Frontier(spec, np.array(block))
        assert len(fr.fps()) == cm.LDS and len(fr.fps(True)) == cm.LDS
        return fr
    return cached("full", make)


def slots_for(kind, stored, fr, slack=7):
    n = 2 * (stored + fr.total()) + slack
    return n + (n & 1) if kind == K_FIRST_C8 else n | 1      # even for the compact table, odd otherwise


def image(kind, nslots, preload):
    """preload {fp: claim} as a table image (the compact table keeps the fps only)."""
    return cm.table_image(nslots, kind, {fp: ~c & M64 for fp, c in preload.items()})


def same(got, want, what):
    got, want = [int(x) for x in got], [int(x) for x in want]
    assert len(got) == len(want), (what, len(got), len(want))
    d = [k for k in range(len(got)) if got[k] != want[k]]
    assert not d, (what, f"{len(d)} differ, first at {d[0]} (tile {d[0] // TILE}): got {got[d[0]]:#x} want {want[d[0]]:#x}")


def check_counters(r, fr, base, check_deadlock, probes, lds_overflow=False, copies=None):
    assert r.overflow == 0, "overflow"
    assert r.act_gen == fr.act_gen(), "act_gen"
    assert r.err_key == fr.err_key(base, check_deadlock), ("err_key", hex(r.err_key))
    if lds_overflow:
        assert probes <= r.probes <= copies, ("probes", r.probes, probes, copies)
    else:
        assert r.probes == probes, ("probes", r.probes, probes)


def check_table(kind, r, want, small=1 << 15):
    got = cm.table_entries(r.table, kind)
    assert set(got) == set(want), ("table fingerprints", len(set(got) - set(want)), len(set(want) - set(got)))
    if kind != K_FIRST_C8:
        bad = [fp for fp in want if got[fp] != want[fp]]
        assert not bad, ("claim words", len(bad), hex(bad[0]), hex(got[bad[0]]), hex(want[bad[0]]))
    if len(r.table) <= small:
        cm.check_runs(r.table, kind)


def run(kind, fr, preload=None, base=0, spread=768, check_deadlock=1, flags=0, cfg=None, **kw):
    """One launch set on fr with `preload` in the table, checked against the model; returns the Result."""
    preload = preload or {}
    nslots = slots_for(kind, len(preload), fr)
    rc, r = cm.selftest(kind, cfg or fr.spec.cfg, fr, base=base, level=LEVEL, check_deadlock=check_deadlock,
                        spread=spread, nslots=nslots, table=image(kind, nslots, preload), flags=flags, **kw)
    assert rc == 0, (rc, kubecheck.load().kc_last_error())
    check_result(kind, r, fr, preload, base, check_deadlock, flags)
    return r


def check_result(kind, r, fr, preload, base, check_deadlock, flags=0):
    mask, final, probes = cm.exact(fr, preload, LEVEL, base)
    check_counters(r, fr, base, check_deadlock, probes)
    if kind == K_EXACT:
        same(r.newmask, mask, "newmask")
        same(r.ttot, cm.tile_popcounts(mask), "tile_total")
        check_table(kind, r, {fp: ~c & M64 for fp, c in final.items()})
        assert r.ovf_count == r.cand_ovf, ("overflow list", r.ovf_count, r.cand_ovf)
        assert all(int(x) <= cm.RCAP for x in r.rcount), "rcount"
    else:
        cm.check_first(fr, set(preload), r.newmask)
        tt = cm.tile_popcounts(r.newmask)
        same(r.ttot, tt, "ttot")
        same(r.rcount, [0] * fr.tiles, "rcount")
        if flags & cm.PF_CSUM:
            same(r.csum, cm.chunk_sums(tt), "csum")
        # (no claim word is written in first-claim mode)
        check_table(kind, r, {fp: ~preload[fp] & M64 if fp in preload else 0 for fp in set(preload) | fr.fps()})
        assert r.ovf_count == 0 and r.settles == 0 and r.cand_ovf == 0


def older(fps, g, level=LEVEL - 2):
    """Claims of an earlier level for the fingerprints."""
    return {fp: cm.make_claim(level, int(g.integers(0, 1 << 30)) << 8 | 3) for fp in fps}


# ----------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 1025])
def test_sizes_preloads_and_bases(n, oracle):
    fr = take(np2_level(oracle), range(700, 700 + n))
    g = np.random.default_rng(n)
    fps = sorted(fr.fps())
    half = older([fp for fp in fps if g.random() < 0.5], g)
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        run(kind, fr)
        run(kind, fr, half)
        for base in (256, 1000):
            run(kind, fr, half, base=base)
    # same-level claims of parents below the chunk start stay and win (CL_LOST);
    # the rest of the fingerprints are new or old as before
    low = {fp: cm.make_claim(LEVEL, int(g.integers(0, 1000)) << 8 | 2) for fp in fps[::3]}
    r = run(K_EXACT, fr, {**half, **low}, base=1000)
    assert not any((int(r.newmask[i]) >> t) & 1 for i, t, fp, _ in fr.copies() if fp in low)
    # same-level claims of this chunk's own later copies (what a tile that ran
    # first would have stored): the smallest copy is a candidate, displaces the
    # claim in settle pass A and clears the displaced copy's bit at parent - base
    last = {}
    for i, t, fp, _ in fr.copies():
        last.setdefault(fp, []).append((i, t))
    for base in (256, 1000):
        late = {fp: cm.make_claim(LEVEL, (base + c[-1][0]) << 8 | c[-1][1]) for fp, c in last.items() if len(c) > 1}
        assert late or n == 1
        r = run(K_EXACT, fr, {**half, **late}, base=base)
        assert r.settles >= len(set(late) - set(half))


# ------------------------------------------------------------ cross-tile copies
@pytest.mark.parametrize("spread", [0, 3, 768])
def test_cross_tile_duplicates(spread, oracle):
    """A 256-parent block in 8 tiles: every fingerprint has a copy in every
    tile; spread 3 makes spread_tile a non-identity at 8 tiles.  In exact mode
    the first tile's copies win whatever the tile order."""
    fr = take(np2_level(oracle), list(range(256)) * 8)
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        r = run(kind, fr, spread=spread)
        if kind == K_EXACT:
            assert not any(int(x) for x in r.newmask[TILE:]) and any(int(x) for x in r.newmask[:TILE])
    run(K_EXACT, fr, spread=spread, base=256)


# ---------------------------------------------------------- forced candidates
def test_forced_candidates_overflow_list(oracle):
    """Every successor fingerprint pre-loaded with a claim of this level under
    rank field 1: larger than any rank-0 key and not 'mine', so every tile
    representative is a candidate (CL_CUR), and a tile keeps only its first
    256: the rest go through the overflow list, pass A's extra blocks and
    k_settle_ovf<1>."""
    fr = take(np2_level(oracle), range(1025))
    g = np.random.default_rng(5)
    foreign = {fp: cm.make_claim(LEVEL, 1 << cm.RANK_SHIFT | int(g.integers(0, 1 << 30))) for fp in fr.fps()}
    reps = [len(d) for d in fr.tile_fps()]
    assert all(k > cm.RCAP for k in reps[:4]) and reps[4] <= 32, reps
    for base in (0, 256):
        r = run(K_EXACT, fr, foreign, base=base)
        same(r.rcount, [min(k, cm.RCAP) for k in reps], "rcount")
        spilled = sum(max(0, k - cm.RCAP) for k in reps)
        assert r.ovf_count == spilled and r.cand_ovf == spilled, (r.ovf_count, r.cand_ovf, spilled)
        assert r.settles >= sum(reps)
        assert sum(cm.popcount(m) for m in r.newmask) == len(fr.fps())     # every fingerprint displaced once


# --------------------------------------------------------------- LDS table full
@pytest.mark.parametrize("tiles", [1, 2])
def test_lds_table_exactly_full(tiles, oracle):
    """2,048 distinct fingerprints in the 2,048-entry LDS table: every probe
    run wraps, nothing overflows."""
    fr = take(full_block(oracle), list(range(256)) * tiles)
    g = np.random.default_rng(tiles)
    some = older(sorted(fr.fps())[::5], g)
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        r = run(kind, fr)
        assert r.probes == cm.LDS * tiles
        run(kind, fr, some, base=256)


# ------------------------------------------------------------------- chunk sums
@pytest.mark.parametrize("kind,n", [(K_FIRST, 16500), (K_FIRST_C8, 32900)])
def test_chunk_sums(kind, n, oracle):
    """65 and 129 tiles: a whole chunk of 64 tiles (two) and a last chunk of one tile, itself partial."""
    lv = np2_level(oracle)
    fr = take(lv, [k % lv.n for k in range(n)])
    assert fr.tiles in (65, 129) and n % TILE
    r = run(kind, fr, flags=cm.PF_CSUM, spread=768 if kind == K_FIRST else 0)
    assert len(r.csum) == (2 if fr.tiles == 65 else 3) and sum(int(x) for x in r.csum) == len(fr.fps())


# ------------------------------------------------------------------ error keys
def test_assert_parent(oracle):
    ocfg = oracle.config(variant=3)
    ref = oracle.run(ocfg)
    fr = cm.Frontier(kubecheck.Spec(kubecheck.ModelConfig(variant=3)), oracle.level_tuples(ocfg, ref["err_level"]))
    bad = [i for i in range(fr.n) if fr.parent(i).fail_pos is not None]
    assert bad and fr.n > 2 * TILE
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        r = run(kind, fr, base=256)
        assert r.err_key == (256 + bad[0]) << 16 | fr.parent(bad[0]).fail_pos << 8 | cm.E_ASSERT


def test_deadlocked_parent(oracle):
    ocfg = oracle.config(ns=0)
    cfg = kubecheck.ModelConfig(ns=0)
    fr = cm.Frontier(kubecheck.Spec(cfg), oracle.level_tuples(ocfg, oracle.run(ocfg)["err_level"]))
    dead = [i for i in range(fr.n) if not fr.parent(i).succ]
    assert dead
    r = run(K_EXACT, fr, base=1000, check_deadlock=1)
    assert r.err_key == (1000 + dead[0]) << 16 | cm.E_DEADLOCK
    r = run(K_EXACT, fr, base=1000, check_deadlock=0)
    assert r.err_key == M64


# --------------------------------------------------------------------- deferred
def run_deferred(kind, prev, links, preload, base, prev_counts):
    spec = prev.spec
    d = cm.deferred(prev, links)
    fr = cm.Frontier(spec, np.array(d["tuples"]))
    nslots = slots_for(kind, len(preload), fr)
    flags = cm.PF_DEFER | (cm.PF_PREV_COUNTS if prev_counts else 0)
    rc, r = cm.selftest(kind, spec.cfg, base=base, level=LEVEL, nslots=nslots,
                        table=image(kind, nslots, preload), flags=flags, prev=prev, links=links)
    assert rc == 0, (rc, kubecheck.load().kc_last_error())
    check_result(kind, r, fr, preload, base, 1)
    W = r.W
    same(r.dfout[:base * W], [cm.GUARD] * (base * W), "df.out below base")
    same(r.dfout[base * W:], fr.packed(), "df.out")
    same(r.counts_out[:base], [cm.GUARD] * base, "counts_out below base")
    same([cm.plan_sum(w) for w in r.counts_out[base:]], [len(fr.parent(i).succ) for i in range(fr.n)], "counts_out")
    assert r.act_dist == d["act_dist"], "act_dist"
    assert r.next_cand == fr.total(), "next_cand"
    assert r.defer_flags == d["defer_flags"] and r.defer_inv_n == d["defer_inv_n"], (r.defer_flags, hex(r.defer_inv_n))
    return r


def test_deferred_frontier(oracle):
    """prev = NP=2 level 12; the links are all of its new successors in BFS order."""
    ocfg = oracle.config(np_=2)
    spec = kubecheck.Spec(kubecheck.ModelConfig(np=2))
    prev = cm.Frontier(spec, oracle.level_tuples(ocfg, 12))
    new = {t.tobytes() for t in oracle.level_tuples(ocfg, 13)}
    links, seen = [], set()
    for i in range(prev.n):
        for t, s in enumerate(prev.parent(i).succ):
            k = s[1].tobytes()
            if k in new and k not in seen:
                seen.add(k)
                links.append((i, t))
    assert len(links) == len(new) and len(links) % TILE and len(links) > TILE
    g = np.random.default_rng(3)
    fr = cm.Frontier(spec, np.array(cm.deferred(prev, links)["tuples"]))
    half = older([fp for fp in sorted(fr.fps()) if g.random() < 0.5], g)
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        for pc in (0, 1):
            run_deferred(kind, prev, links, half, 0, pc)
        run_deferred(kind, prev, links, {}, 256, 1)


def test_deferred_invariant_violation(oracle, fixtures):
    """The variant-1 NoLostUpdate violator rebuilt inside k_claim: DF_INVARIANT and ~(its index)."""
    trace = fixtures["variant1_lost_update"]["trace"]
    cfg = kubecheck.ModelConfig(variant=1, invariants=7)
    spec = kubecheck.Spec(cfg)
    assert spec.check_invariants(trace[-1]) == "NoLostUpdate"
    prev_tuples = np.array([trace[-3], trace[-2]], dtype=U64)
    prev = cm.Frontier(spec, prev_tuples)
    links = [(pp, t) for pp in (0, 1) for t in range(len(prev.parent(pp).succ))]
    d = cm.deferred(prev, links)
    assert d["defer_flags"] == cm.DF_INVARIANT and 0 < (~d["defer_inv_n"] & M64) < len(links)
    for kind in (K_EXACT, K_FIRST, K_FIRST_C8):
        run_deferred(kind, prev, links, {}, 0, 1)
    # with NoLostUpdate off the same links raise nothing
    quiet = cm.Frontier(kubecheck.Spec(kubecheck.ModelConfig(variant=1, invariants=3)), prev_tuples)
    assert [len(p.succ) for p in quiet.block] == [len(p.succ) for p in prev.block]
    r = run_deferred(K_EXACT, quiet, links, {}, 0, 0)
    assert r.defer_flags == 0


# ---------------------------------------------------------------------- sharded
def run_sharded(fr, world, rank, preload=None, stage_cap=None, lds_overflow=False):
    preload = preload or {}
    reps, remote = cm.representatives(fr, rank, world)
    need = sum(len(x) for x in (remote if lds_overflow else reps))
    cap = need + 5 if stage_cap is None else stage_cap
    nslots = slots_for(K_SHARD, len(preload), fr)
    rc, r = cm.selftest(K_SHARD, fr.spec.cfg, fr, level=LEVEL, nslots=nslots, table=image(K_SHARD, nslots, preload),
                        world=world, rank=rank, stage_cap=cap)
    assert rc == 0, (rc, kubecheck.load().kc_last_error())
    mask, final, probes = cm.exact(fr, preload, LEVEL, 0, rank, world)
    owned = sum(1 for _, _, fp, _ in fr.copies(True) if cm.owner(fp, world) == rank)
    check_counters(r, fr, 0, 1, probes, lds_overflow, owned)
    same(r.newmask, mask, "newmask")
    same(r.ttot, cm.tile_popcounts(mask), "tile_total")
    check_table(K_SHARD, r, {fp: ~c & M64 for fp, c in final.items()})
    # repmask: the representatives; with an LDS overflow also copies that missed the table
    rep_m, rem_m = cm.masks_of(sum(reps, []), fr.n), cm.masks_of(sum(remote, []), fr.n)
    got = [int(x) for x in r.repmask]
    if lds_overflow:
        assert all(a & ~b == 0 for a, b in zip(rep_m, got)), "repmask misses a representative"
        assert all(a & ~b == 0 for a, b in zip(got, rem_m)), "repmask marks a copy no other rank owns"
    else:
        same(got, rep_m, "repmask")
    staged = cm.staged_records(fr, got, rank, world)
    cnt = np.zeros((world, fr.n), dtype=np.int64)
    tcnt = np.zeros((world, fr.tiles), dtype=np.int64)
    for tile, recs in enumerate(staged):
        for o, words in recs:
            cnt[o][(words[-1] >> 16) & 0xffffffff] += 1
            tcnt[o][tile] += 1
    same(r.cnt, cnt.reshape(-1), "cnt")
    same(r.tcnt, tcnt.reshape(-1), "tcnt")
    total = int(tcnt.sum())
    assert r.stage_cur == total, ("stage_cur", r.stage_cur, total)
    # the segments: disjoint, inside [0, stage_cur), each holding its tile's records in order
    W = r.W
    taken = np.zeros(max(total, 1), dtype=np.int64)
    refused = []
    for tile, recs in enumerate(staged):
        off = int(r.stoff[tile])
        if off == M64:
            refused.append(tile)
            continue
        if not recs:
            assert off == 0, ("stoff of a tile without records", tile, off)
            continue
        assert off + len(recs) <= min(total, cap), ("segment past the records reserved", tile, off)
        taken[off:off + len(recs)] += 1
        got_recs = r.records[off * (W + 1):(off + len(recs)) * (W + 1)]
        same(got_recs, sum((w for _, w in recs), []), f"records of tile {tile}")
    assert taken.max() <= 1, "segments overlap"
    if total <= cap:
        assert not refused and r.defer_flags == 0 and (total == 0 or taken.min() == 1)
    else:
        assert refused and r.defer_flags == cm.DF_STAGE, (refused, r.defer_flags)
        assert all(staged[t] for t in refused)
    return r, tcnt


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_sharded_natural_tiles(world, oracle):
    lv = np2_level(oracle)
    g = np.random.default_rng(world)
    for n in (1, 256, 257, 1025):
        fr = take(lv, range(1200, 1200 + n))
        half = older([fp for fp in sorted(fr.fps(True)) if g.random() < 0.5], g)
        for rank in range(world):
            r, tcnt = run_sharded(fr, world, rank)
            if n == 1 and world == 8:
                assert (tcnt[:, 0] == 0).sum() > 1          # an owner without a record in the tile: tt[o] == 0
            if rank == world - 1:
                run_sharded(fr, world, rank, half)


def test_sharded_stage_buffer_too_small(oracle):
    fr = take(np2_level(oracle), range(1025))
    reps, _ = cm.representatives(fr, 1, 3)
    need = sum(len(x) for x in reps)
    assert all(reps[:4])
    for cap in (need - 1, len(reps[0]), 0):
        r, _ = run_sharded(fr, 3, 1, stage_cap=cap)
        assert r.defer_flags == cm.DF_STAGE


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_lds_overflow(world, oracle):
    """2,048 distinct fingerprints against the sharded tile's 1,792 entries: the
    lds_claim < 0 branch (direct claims of owned copies, remote-owner
    accounting, the dealt parent index).  World 3 takes the owner from the
    fingerprint (owner_of), world 2 from the owner bits.  Model<1,3,1> is the
    only model of the harness whose tile can pass 1,792 distinct fingerprints
    (NP=2 parents have at most 6 distinct successors), and its states are too
    wide for k_claim's deal through LDS (DEAL is false for it), so the dealt
    parent index is the lane's own here: a wrong KC_LP in that branch would not
    show in this test."""
    fr = full_block(oracle)
    assert len(fr.fps(True)) > cm.LDS_SH
    g = np.random.default_rng(world)
    some = older(sorted(fr.fps(True))[::4], g)
    for rank in range(world):
        r, _ = run_sharded(fr, world, rank, lds_overflow=True)
        # a fingerprint the rank owns is new exactly once
        mine = {fp for fp in fr.fps(True) if cm.owner(fp, world) == rank}
        won = [fp for i, t, fp, _ in fr.copies(True) if (int(r.newmask[i]) >> t) & 1]
        assert sorted(won) == sorted(mine)
        run_sharded(fr, world, rank, some, lds_overflow=True)
