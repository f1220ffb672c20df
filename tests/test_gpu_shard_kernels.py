"""The sharded level's kernels (csrc/shard_kernels.h), launched by
kc_shard_selftest with ShardT's grids and block sizes, on inputs made here,
against shard_model.py (plain Python; held to the oracle by
test_shard_model.py).  Integers only: every comparison is equality or a set
relation, every output section carries guards fore and aft that must come back
untouched (shard_model._call), and every case asserts its own precondition on
the host before it touches the device.

Kernel -> test:
  k_owner_tscan, k_owner_cscan, k_owner_scan_small, hipcub through Widen8 +
  k_owner_totals, owner_row, head_to_host
        test_owner_scans_agree_with_one_cumulative_sum, test_small_scan_carries,
        test_owner_scan_of_a_real_level, test_owner_scan_world_1_totals_are_zero,
        test_owner_scan_no_parents, test_owner_row_rules,
        test_owner_scan_without_a_row
  k_shard_gather
        test_gather_shapes, test_gather_of_a_real_level,
        test_pack_and_gather_write_the_same_buffer
  k_shard_pack
        test_pack_of_a_real_level, test_pack_and_gather_write_the_same_buffer
  k_shard_materialize<M, false / true> (shard_rebuild)
        test_rebuild_of_a_real_level, test_rebuild_sizes,
        test_rebuild_reports_an_invariant_violation_through_each_link_kind
  k_undo_gen
        test_undo_takes_back_what_the_level_generated
  k_head_reset, the sharded k_claim, k_rec_claim, k_settle_both<M, 0 / 1>,
  k_ovf_win_scan, k_shard_emit_links (tail 1)
        test_insert_of_a_real_level and every other deterministic case
  k_settle_ovf<1> + k_win_scan, k_shard_cand (tail 0), k_shard_scan_small,
  hipcub + k_shard_base, k_shard_emit on tile counts and on offsets
        test_insert_paths_agree, test_insert_without_own_parents,
        test_insert_without_records
  rec_settle's displacement branches
        test_a_record_displaces_an_own_claim_and_the_other_way,
        test_two_senders_one_fingerprint_in_both_arrival_orders,
        test_a_record_of_an_older_levels_fingerprint_is_out
  emit_rec_block's invariant check
        test_an_invariant_violating_record_gives_the_error_key
  TLC-order claim keys (k_claim TLC, record_ckey, ClaimKeys::mine)
        test_tlc_order_keys_find_the_same_states
  k_shard_emit_links' wave loop and capacity rerun
        test_emit_links_wave_loop_and_capacity
  k_claim FIRST sharded, k_rec_claim_first (16-B slots, compact), k_win_scan
        test_first_claim_insert
  k_tlc_mask, k_tlc_pos, k_tlc_perm, the two NewCount scans
        test_tlc_word_edges, test_tlc_sizes, test_tlc_overflow_keys,
        test_tlc_kernels_reproduce_the_oracles_order

Not reached: k_shard_spill_queries / k_shard_spill_apply; shard_narrow.h (the
device-driven narrow levels); shard_driver.hip's k_multi_copy / k_sum_u32; a
full seen-set (CL_FULL) in k_rec_claim / k_rec_claim_first; the candidate
overflow list with entries on this path (the list is empty on these levels:
its passes run over nothing; test_gpu_claim.py fills it for k_settle_ovf); a
same-level claim pre-loaded by another rank's record; world 15 through the
insert (the claim harness and these levels stop at 8; the scans, the gather
and the pack run at 15); the record layout itself, which is compared through
the product's host-side record_pack / record_unpack, not a model of the bits;
DF_STAGE's fallback inside ShardT::pack (the hipcub scan + k_shard_pack pair
is driven, the decision is not).  Those are still reached only end to end
(test_gpu_shard.py, test_gpu_shard_seenspill.py)."""
import numpy as np
import pytest

import claim_model as cm
import kubecheck
import shard_model as sm
from claim_model import M64
from shard_model import CSUM_TILES, GUARD, GUARD32

pytestmark = pytest.mark.gpu

U64 = np.uint64
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def np2_level(oracle, world, tlc=False):
    """NP=2 level 22 (3,819 parents) as a sharded level of the model; the
    frontier and the seen fingerprints are computed once."""
    def base():
        ocfg = oracle.config(np_=2)
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=2))
        seen = {spec.fingerprint_own(t) for k in range(1, 23) for t in oracle.level_tuples(ocfg, k)}
        return spec, cm.Frontier(spec, oracle.level_tuples(ocfg, 22)), seen, oracle.level_tuples(ocfg, 23)
    spec, whole, seen, nxt = cached("np2", base)
    return cached(("np2", world, tlc), lambda: sm.Level(spec, None, seen, world, tlc=tlc, whole=whole)), nxt


def np2_seen(oracle):
    """The owner-projected fingerprints of NP=2 levels 1 to 22."""
    np2_level(oracle, 2)
    return _cache["np2"][2]


# ------------------------------------------------------------------ owner scans
MODES = (0, 1, 2, 3)            # k_owner_tscan, k_owner_cscan, k_owner_scan_small, hipcub + k_owner_totals
HEAD = dict(err_key=0x1234 << 16 | 1, chunk_base=11, overflow=0, batch_used=0, cand_total=12, level_new=13,
            emit_done=14, defer_flags=4, defer_inv_n=15, defer_err=M64)


def check_owner_scan(mode, world, T, cells, **kw):
    """One launch against the cumulative sum; returns the Result."""
    rc, r = sm.owner_scan(mode, world, T, cells, head=HEAD, status_new=7, status_err=M64 - 5, **kw)
    assert rc == 0
    n = world * T
    off, tot = sm.owner_offsets(cells, world)
    if world == 1 and mode == 3:
        assert (r.off == U64(GUARD32)).all(), "ShardT scans nothing at world 1"
    else:
        assert [int(x) for x in r.off[:n]] == [int(x) for x in off]
    if mode < 2:
        # the tile scan stores whole 16-B groups and the total behind the last cell
        assert int(r.off[n]) == sum(cells)
        assert (r.off[max(4 * ((n + 3) // 4), n + 1):] == U64(GUARD32)).all()
    want = [t if world > 1 else 0 for t in tot] + [0] * (16 - world)
    assert [int(x) for x in r.tot] == want
    assert [int(x) for x in r.host_tot] == want
    hw = [HEAD[k] for k in sm.HEAD_WORDS]
    assert [int(r.host_head[k]) for k in sm.HEAD_COPIED] == [hw[k] for k in sm.HEAD_COPIED]
    assert int(r.host_head[6]) == GUARD and int(r.host_head[8]) == GUARD
    if kw.get("want_row", 1):
        assert [int(x) for x in r.row] == sm.owner_row(want[:world], world, HEAD, 7, M64 - 5, 0, M64)
    else:
        assert (r.row == U64(GUARD)).all()
    # k_owner_cscan zeroes its sums for the next level; nobody else writes the counts
    assert [int(x) for x in r.cells_after] == ([0] * n if mode == 1 else list(cells))
    return r


def counts_for(world, T, empty=(), seed=1, top=9):
    rng = np.random.default_rng(seed * 1000 + world * 37 + T)
    c = rng.integers(0, top, size=(world, T))
    for o in empty:
        c[o, :] = 0
    return [int(x) for x in c.reshape(-1)]


@pytest.mark.parametrize("world", [2, 3, 8, 15])
@pytest.mark.parametrize("T", [1, 4, 5, 1023, 1025])
def test_owner_scans_agree_with_one_cumulative_sum(world, T):
    """All four spellings on the same counts: the offsets are one cumulative
    sum over the owner-major cells, the totals its owner sums.  T = 4 / 5: a
    whole 16-B group and one cell more; 1023 / 1025: either side of one cell
    per thread of the small scan's first pass and of a tile scan group."""
    empties = [(), (0,), (world - 1,), (world // 2,)]
    for k, empty in enumerate(empties):
        cells = counts_for(world, T, empty, seed=k)
        if empty:
            assert sum(cells[empty[0] * T:(empty[0] + 1) * T]) == 0, "this owner has zero records"
        for mode in MODES:
            if mode == 2 and world * T > sm.OWNER_SMALL_SCAN:
                continue
            r = check_owner_scan(mode, world, T, cells)
            if empty:
                assert int(r.tot[empty[0]]) == 0


def test_owner_scan_world_1_totals_are_zero():
    cells = counts_for(1, 300)
    assert sum(cells) > 0
    for mode in MODES:
        r = check_owner_scan(mode, 1, 300, cells)
        assert not r.tot.any() and not r.host_tot.any() and int(r.row[0]) == 0


@pytest.mark.parametrize("world,n", [(3, 341), (2, 512), (5, 205), (3, 683), (5, 820)])
def test_small_scan_carries(world, n):
    """k_owner_scan_small takes 1,024 cells a pass: 1,023 cells (one short of
    a pass), 1,024, 1,025 (one cell into the second), 2,049 and 4,100 (the
    carry of a carry).  Every cell is 255, so a lost carry cannot hide in
    zeros."""
    assert world * n in (1023, 1024, 1025, 2049, 4100)
    cells = [255] * (world * n)
    for mode in (2, 3):
        r = check_owner_scan(mode, world, n, cells)
        assert int(r.off[-1]) == 255 * (world * n - 1)


def test_owner_scan_no_parents():
    for mode in (2, 3):
        r = check_owner_scan(mode, 4, 0, [])
        assert not r.tot.any() and [int(x) for x in r.row] == [0, 0, 0, 0, 7, M64 - 5, 0]


@pytest.mark.parametrize("mode", MODES)
def test_owner_row_rules(mode):
    """status_err: a deferred invariant key below it wins; a level-1 Init error
    overrides both; the failure word follows overflow and batch_used."""
    world, T = 3, 6
    cells = counts_for(world, T)
    tot = sm.owner_offsets(cells, world)[1]
    cases = [
        (dict(defer_err=100), 200, 0, M64, 100, 0),                 # the deferred key is smaller
        (dict(defer_err=300), 200, 0, M64, 200, 0),                 # ... is larger
        (dict(defer_err=M64), M64, 0, M64, M64, 0),                 # no error anywhere
        (dict(defer_err=100), 200, 1, 0x30012, 0x30012, 0),         # level 1: the Init error, though it is larger
        (dict(defer_err=100), 200, 0, 0x30012, 100, 0),             # an Init key is level 1's alone
        (dict(defer_err=100), 200, 1, M64, 100, 0),                 # level 1 without one
        (dict(defer_err=M64, overflow=1), M64, 0, M64, M64, 1),
        (dict(defer_err=M64, batch_used=5), M64, 0, M64, M64, 1),
    ]
    for head, status_err, level1, init_err, want_err, want_fail in cases:
        assert sm.owner_row(tot, world, {"overflow": 0, "batch_used": 0, **head}, 9, status_err, level1,
                            init_err)[world:] == [9, want_err, want_fail]
        rc, r = sm.owner_scan(mode, world, T, cells, head=head, status_new=9, status_err=status_err, level1=level1,
                              init_err=init_err)
        assert rc == 0
        assert [int(x) for x in r.row] == tot + [9, want_err, want_fail]
        assert int(r.host_head[9]) == head["defer_err"] and int(r.host_head[2]) == head.get("overflow", 0)


@pytest.mark.parametrize("mode", MODES)
def test_owner_scan_without_a_row(mode):
    check_owner_scan(mode, 8, 37, counts_for(8, 37), want_row=0)


@pytest.mark.parametrize("world", [2, 3, 8, 15])
def test_owner_scan_of_a_real_level(oracle, world):
    """NP=2 level 22, the rank with the most records to send: its tile counts
    through k_owner_tscan, their chunk sums through k_owner_cscan; the totals
    are what the model sends to each owner."""
    L, _ = np2_level(oracle, world)
    rk = max(L.ranks, key=lambda r: sum(len(g) for g in r.send))
    T = rk.fr.tiles
    assert T >= 1 and sum(len(g) for g in rk.send) > 0 and not rk.send[rk.rank]
    cells = [c for row in rk.tcnt for c in row]
    r = check_owner_scan(0, world, T, cells)
    assert [int(x) for x in r.tot[:world]] == [len(g) for g in rk.send]
    csum = [s for row in rk.tcnt for s in cm.chunk_sums(row)]
    r = check_owner_scan(1, world, len(csum) // world, csum)
    assert [int(x) for x in r.tot[:world]] == [len(g) for g in rk.send]


# ----------------------------------------------------------------------- gather
def synthetic_stage(world, T, tcnt, rw, holes=()):
    """A staging buffer for tcnt[o][tile]: tiles staged in a shuffled order (as
    the device's cursor hands segments out), every word naming its tile, owner,
    record and word, so any misplaced 16-B unit shows.  Tiles in `holes` stage
    nothing (stoff ~0)."""
    order = list(range(T))
    np.random.default_rng(T * 16 + world).shuffle(order)
    stoff, stage, at = [M64] * T, [], 0
    for t in order:
        if t in holes:
            continue
        stoff[t] = at
        for o in range(world):
            for k in range(tcnt[o][t]):
                stage += [(t << 40) | (o << 32) | (k << 8) | w for w in range(rw)]
                at += 1
    return stoff, stage


def run_gather(np_, world, T, tcnt, holes=()):
    cfg = kubecheck.ModelConfig(np=np_)
    rw = sm.RW[np_]
    stoff, stage = synthetic_stage(world, T, tcnt, rw, holes)
    flat = [c for row in tcnt for c in row]
    toff, _ = sm.owner_offsets(flat, world)
    csum = [s for row in tcnt for s in cm.chunk_sums(row)]
    coff, _ = sm.owner_offsets(csum, world)
    want = sm.send_buffer(stage, stoff, tcnt, world, rw)
    assert len(want) == sum(flat) * rw
    got = []
    for chunked, offs in ((0, toff), (1, coff)):
        rc, buf = sm.gather(cfg, world, T, chunked, stage, stoff, flat, offs)
        assert rc == 0
        assert [GUARD if w is None else w for w in want] == [int(x) for x in buf], ("chunked", chunked)
        got.append(buf)
    assert (got[0] == got[1]).all()


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129])
def test_gather_shapes(np_, T):
    """T = 64 / 65 / 129: whole chunks and a last chunk of one tile (tile index
    0 of its chunk; tile 63 is the last lane of the wave prefix).  World 15;
    tiles that staged nothing; tiles with records for one owner only; an owner
    with no records at all."""
    world = 15
    rng = np.random.default_rng(T)
    tcnt = [[int(x) for x in rng.integers(0, 6, size=T)] for _ in range(world)]
    tcnt[14] = [0] * T                                          # owner 14 has zero records
    one = {t: int(rng.integers(0, 14)) for t in range(0, T, 5)}   # these tiles send to one owner only
    for t, o in one.items():
        for k in range(world):
            tcnt[k][t] = 7 if k == o else 0
    holes = set(range(2, T, 7)) - {T - 1}
    for t in holes:
        for k in range(world):
            tcnt[k][t] = 0
    assert sum(tcnt[14]) == 0 and one and all(sum(tcnt[k][t] for k in range(world)) == 7 for t in one if t not in holes)
    if T >= 64:
        assert sum(tcnt[k][63] for k in range(world)) > 0 and 63 not in holes, "tile 63 of chunk 0 sends records"
    if T in (65, 129):
        assert (T - 1) % CSUM_TILES == 0 and sum(tcnt[k][T - 1] for k in range(world)) > 0 and T - 1 not in holes
    run_gather(np_, world, T, tcnt, holes)
    run_gather(np_, 2, T, tcnt[:2])


@pytest.mark.parametrize("world", [2, 8])
def test_gather_of_a_real_level(oracle, world):
    """The tile counts of NP=2 level 22 at the rank that sends most."""
    L, _ = np2_level(oracle, world)
    rk = max(L.ranks, key=lambda r: sum(len(g) for g in r.send))
    assert rk.fr.tiles > 1
    run_gather(2, world, rk.fr.tiles, rk.tcnt)


# ------------------------------------------------------------------------- pack
def model_rows(spec, groups):
    """The model's send buffer as rows of state words + key, owner by owner."""
    return [[int(w) for w in spec.pack(rec.tuple)] + [rec.key] for g in groups for rec in g]


def pack_inputs(rk):
    reps = [e for tile in rk.reps for e in tile]
    repmask = cm.masks_of(reps, rk.fr.n)
    return reps, repmask


@pytest.mark.parametrize("world,tlc", [(2, False), (3, False), (8, False), (15, False), (3, True)])
def test_pack_of_a_real_level(oracle, world, tlc):
    """k_shard_pack on a rank of NP=2 level 22 writes the model's send buffer:
    grouped by owner, each group in (parent, position) order, keys carrying the
    local parent index, or its G under TLC order."""
    L, _ = np2_level(oracle, world, tlc)
    rk = max(L.ranks, key=lambda r: sum(len(g) for g in r.send))
    reps, repmask = pack_inputs(rk)
    n = rk.fr.n
    assert n % 256 != 0 and n > 256, "a partial last block, more than one block"
    assert any(m == 0 for m in repmask), "a parent with nothing to send"
    by_parent = {}
    for i, t, a, o in reps:
        by_parent.setdefault(i, []).append(o)
    assert any(len(os) >= 2 and len(set(os)) == 1 for os in by_parent.values()), \
        "a parent whose marked successors all go to one owner"
    if tlc:
        assert any(g != i for i, g in enumerate(rk.G)), "G differs from the local index"
    rc, r = sm.pack(L.spec.cfg, rk.fr.packed(), n, repmask, world, rk.rank, gpos=rk.G if tlc else None)
    assert rc == 0
    assert r.per_owner == [len(g) for g in rk.send] and r.per_owner[rk.rank] == 0
    assert [[int(w) for w in row] for row in r.records] == model_rows(L.spec, rk.send)


@pytest.mark.parametrize("world", [2, 8])
def test_pack_and_gather_write_the_same_buffer(oracle, world):
    """The two ways to a send buffer: k_claim's staged records through
    k_shard_gather (chunked and not), and k_shard_pack re-expanding the marked
    successors: byte-identical."""
    L, _ = np2_level(oracle, world)
    rk = max(L.ranks, key=lambda r: sum(len(g) for g in r.send))
    reps, repmask = pack_inputs(rk)
    total = len(reps)
    cfg = L.spec.cfg
    rc, c = cm.selftest(cm.K_SHARD, cfg, rk.fr, level=23, nslots=2 * (rk.fr.total() + 1), world=world, rank=rk.rank,
                        stage_cap=total + 64)
    assert rc == 0 and c.defer_flags & cm.DF_STAGE == 0
    assert [int(m) for m in c.repmask] == repmask
    T = rk.fr.tiles
    tcnt = [int(x) for x in c.tcnt]
    assert tcnt == [x for row in rk.tcnt for x in row]
    toff, _ = sm.owner_offsets(tcnt, world)
    coff, _ = sm.owner_offsets([s for row in rk.tcnt for s in cm.chunk_sums(row)], world)
    stoff = [int(x) for x in c.stoff]
    rc, p = sm.pack(cfg, rk.fr.packed(), rk.fr.n, repmask, world, rk.rank)
    assert rc == 0 and len(p.raw) == total * sm.RW[2]
    for chunked, offs in ((0, toff), (1, coff)):
        rc, buf = sm.gather(cfg, world, T, chunked, c.stage, stoff, tcnt, offs)
        assert rc == 0 and (buf == p.raw).all(), ("chunked", chunked)


# ---------------------------------------------------------------------- rebuild
def rebuild_case(L, rk):
    spec = L.spec
    rows = [[int(w) for w in spec.pack(rec.tuple)] + [rec.key] for rec in rk.recv]
    want = [[int(w) for w in spec.pack(x)] for x in rk.next]
    cand = sum(len(cm.Parent(spec, x).succ) for x in rk.next)
    return rows, want, cand


@pytest.mark.parametrize("tlc", [False, True])
@pytest.mark.parametrize("prev_counts", [0, 1])
def test_rebuild_of_a_real_level(oracle, tlc, prev_counts):
    """k_shard_materialize on the links of a rank of NP=2 level 22 at world 3:
    own links (parent << 8 | position) and record links (bit 63 | index into
    the receive buffer) mixed; the states are the model's next states, in order."""
    L, _ = np2_level(oracle, 3, tlc)
    rk = L.ranks[1]
    own = [lk for lk in rk.link if not lk & sm.LINK_REC]
    assert own and len(own) < len(rk.link), "links of both kinds"
    assert len(rk.link) > 257
    rows, want, cand = cached(("rebuild", tlc), lambda: rebuild_case(L, rk))
    rc, r = sm.materialize(L.spec.cfg, rk.fr.packed(), rk.fr.n, rk.link, rows, rank=rk.rank,
                           prev_gpos=rk.G if tlc else None, prev_counts=prev_counts)
    assert rc == 0
    assert [[int(w) for w in s] for s in r.states] == want
    assert r.act_dist == rk.act_dist and r.next_cand == cand and r.defer_err == M64


@pytest.mark.parametrize("n", [1, 256, 257])
def test_rebuild_sizes(oracle, n):
    """One state, one full block, one block and one thread; the links taken
    from the end of the level, so a lone state is a record's."""
    L, _ = np2_level(oracle, 3)
    rk = L.ranks[1]
    rows, want, _ = cached(("rebuild", False), lambda: rebuild_case(L, rk))
    links = rk.link[-n:]
    assert links[-1] & sm.LINK_REC, "the level ends with a record's state"
    rc, r = sm.materialize(L.spec.cfg, rk.fr.packed(), rk.fr.n, links, rows, rank=rk.rank)
    assert rc == 0 and [[int(w) for w in s] for s in r.states] == want[-n:]
    assert sum(r.act_dist) == n


@pytest.mark.parametrize("tlc", [False, True])
def test_rebuild_reports_an_invariant_violation_through_each_link_kind(fixtures, tlc):
    """The variant-1 NoLostUpdate violator as an own successor and as a record:
    defer_err is the key the materialising emit would have made (the parent
    field: the local index, or G under TLC order, where the rank is dropped)."""
    trace = fixtures["variant1_lost_update"]["trace"]
    cfg = kubecheck.ModelConfig(variant=1, invariants=7)
    spec = kubecheck.Spec(cfg)
    assert spec.check_invariants(trace[-1]) == "NoLostUpdate"
    prev = cm.Frontier(spec, np.array([trace[-3], trace[-2]], dtype=U64))
    bad = np.array(trace[-1], dtype=U64)
    t_bad = [t for t, s in enumerate(prev.parent(1).succ) if s[1].tobytes() == bad.tobytes()]
    assert len(t_bad) == 1, "the violator is one successor of the trace's last parent"
    t_bad = t_bad[0]
    rank, G = 2, [70000, 70007]
    mask = 0x0fffffffffffff00 if tlc else M64 & ~0xff
    # own link: parent 1, position t_bad, after a clean own link and a clean record
    clean = prev.parent(0).succ[0]
    assert spec.check_invariants(clean[1]) is None
    rec_key = sm.record_key(1, 123456, 7, clean[0])
    rows = [[int(w) for w in spec.pack(clean[1])] + [rec_key]]
    links = [0 << 8 | 0, sm.LINK_REC | 0, 1 << 8 | t_bad]
    rc, r = sm.materialize(cfg, prev.packed(), 2, links, rows, rank=rank, prev_gpos=G if tlc else None)
    assert rc == 0
    assert r.defer_err == (sm.record_key(rank, G[1] if tlc else 1, t_bad) & mask) | cm.E_INVARIANT
    assert [int(w) for w in r.states[2]] == [int(w) for w in spec.pack(bad)]
    # record link: the violator arrives as a record; the own links are clean
    bad_key = sm.record_key(1, 654321, 9, prev.parent(1).succ[t_bad][0])
    rows = [[int(w) for w in spec.pack(bad)] + [bad_key]]
    rc, r = sm.materialize(cfg, prev.packed(), 2, [0 << 8 | 0, sm.LINK_REC | 0], rows, rank=rank,
                           prev_gpos=G if tlc else None)
    assert rc == 0
    assert r.defer_err == (bad_key & mask) | cm.E_INVARIANT
    # with NoLostUpdate off nothing is reported
    quiet = kubecheck.ModelConfig(variant=1, invariants=3)
    rc, r = sm.materialize(quiet, prev.packed(), 2, [0 << 8 | 0, sm.LINK_REC | 0], rows, rank=rank)
    assert rc == 0 and r.defer_err == M64


def test_undo_takes_back_what_the_level_generated(oracle):
    """k_undo_gen subtracts each parent's successors per action, from the plans
    k_claim keeps: after it act_gen is back where it started, also with an
    Assert parent in the level (its successors before the failing action)."""
    L, _ = np2_level(oracle, 3)
    fr = L.ranks[0].fr
    start = [1000 + 3 * k for k in range(cm.NACT)]
    gen = fr.act_gen()
    assert sum(gen) == fr.total() > 0 and fr.n % 256 != 0
    rc, after = sm.undo(L.spec.cfg, fr.packed(), fr.n, [s + g for s, g in zip(start, gen)])
    assert rc == 0 and after == start
    # from zero: the counters wrap, mod 2^64
    rc, after = sm.undo(L.spec.cfg, fr.packed(), fr.n, [0] * cm.NACT)
    assert rc == 0 and after == [(-g) & M64 for g in gen]
    ocfg = oracle.config(variant=3)
    cfg = kubecheck.ModelConfig(variant=3)
    afr = cm.Frontier(kubecheck.Spec(cfg), oracle.level_tuples(ocfg, oracle.run(ocfg)["err_level"]))
    assert any(afr.parent(i).fail_pos is not None for i in range(afr.n))
    gen = afr.act_gen()
    rc, after = sm.undo(cfg, afr.packed(), afr.n, [s + g for s, g in zip(start, gen)])
    assert rc == 0 and after == start


# ----------------------------------------------------------------------- insert
LEVEL = 23                      # the successors' level in every insert case
OLD = cm.make_claim(9, 7)       # an older level's claim


def preload_for(rk, seen):
    """{fp: ~claim} of the seen fingerprints this rank's copies and records hit
    (the rest of the seen-set cannot change what the kernels do)."""
    hit = {fp for _, _, fp, _ in rk.fr.copies(True)} | {rec.fp for rec in rk.recv}
    return {fp: ~OLD & M64 for fp in hit & seen}


def run_insert(kind, spec, rk, seen, world, *, tlc=False, W=0, **kw):
    pre = preload_for(rk, seen)
    nslots = 2 * (len(pre) + rk.fr.total() + len(rk.recv) + 1)
    tk = cm.K_FIRST_C8 if kind == sm.K_INSERT_FIRST and kw.get("path") == 1 else cm.K_EXACT
    table = cm.table_image(nslots, tk, pre if tk == cm.K_EXACT else set(pre))
    rc, r = sm.insert(kind, spec.cfg, rk.fr if rk.fr.n else None, sm.record_rows(spec, rk.recv), level=LEVEL,
                      nslots=nslots, world=world, rank=rk.rank, table=table, gpos=rk.G if tlc else None, W=W, **kw)
    assert rc == 0
    assert r.overflow == 0
    cm.check_runs(r.table, tk)
    r.entries, r.pre, r.tk = cm.table_entries(r.table, tk), pre, tk
    return r


def popcounts(masks):
    return [cm.popcount(m) for m in masks]


def check_insert(r, rk, spec, *, tlc=False, emit=1, path=0, next_gidx=0):
    """Everything a deterministic insert returned against the model's rank."""
    n, nrec = rk.fr.n, len(rk.recv)
    assert [int(m) for m in r.newmask] == rk.newmask
    assert [int(x) for x in r.isnew] == rk.isnew
    assert [int(x) for x in r.rfp] == [rec.fp for rec in rk.recv]
    own_fps = {fp for _, _, fp, _ in rk.fr.copies(True)}
    inserters = {}
    for j, rec in enumerate(rk.recv):
        fl = int(r.flag[j])
        # (a loser's flag depends on what it found stored: out at once behind a
        # smaller claim, else a candidate, an inserter or a displacer that lost later)
        assert fl in (sm.RF_OUT, sm.RF_CAND, sm.RF_INSERTER, sm.RF_DISPLACER)
        if rec.fp in r.pre:
            assert fl == sm.RF_OUT, "an older level's fingerprint"
        if fl == sm.RF_INSERTER:
            assert rec.fp not in own_fps, "k_claim had inserted this fingerprint before any record came"
            inserters[rec.fp] = inserters.get(rec.fp, 0) + 1
        if rk.isnew[j]:
            assert fl == (sm.RF_DISPLACER if rec.fp in own_fps else fl) and fl >= sm.RF_INSERTER
    assert all(k == 1 for k in inserters.values()), "one inserter a fingerprint"
    # the table: what was there, and every new fingerprint under the level's smallest claim
    want = dict(r.pre)
    for fp, c in rk.claims.items():
        want[fp] = ~cm.make_claim(LEVEL, c) & M64
    assert r.entries == want
    assert r.chunk_base == rk.chunk_base and r.level_new == rk.level_new
    total = rk.level_new
    if path == 0:
        cells = r.tiles + r.rgrid
        wt = cm.tile_popcounts(rk.newmask) + [sum(rk.isnew[k:k + 256]) for k in range(0, nrec, 256)]
        assert len(wt) == cells and [int(x) for x in r.wtot[:cells]] == wt
        off, _ = sm.owner_offsets(wt, 1)
        assert [int(x) for x in r.woff[:cells]] == [int(x) for x in off] and int(r.woff[cells]) == total
    else:
        off, _ = sm.owner_offsets(popcounts(rk.newmask), 1)
        assert [int(x) for x in r.offsets] == [int(x) for x in off]
        off, _ = sm.owner_offsets(rk.isnew, 1)
        assert [int(x) for x in r.ioff] == [int(x) for x in off]
    if emit:
        assert [int(x) for x in r.link[:total]] == rk.link
        assert (r.link[total:] == U64(GUARD)).all()
        assert [int(x) for x in r.pkeys[next_gidx:next_gidx + total]] == rk.pkeys
        assert r.err_key == M64 and not any(r.act_dist) and r.cand_total == 0
    else:
        assert [[int(w) for w in s] for s in r.next[:total]] == [[int(w) for w in spec.pack(x)] for x in rk.next]
        assert (r.next[total:] == U64(GUARD)).all()
        # (the materialising emit puts the action into an own winner's key as well)
        acts = [rk.fr.parent(lk >> 8).succ[lk & 0xff][0] for lk in rk.link[:rk.chunk_base]]
        want_keys = [k | a for k, a in zip(rk.pkeys, acts)] + rk.pkeys[rk.chunk_base:]
        assert [int(x) for x in r.pkeys[next_gidx:next_gidx + total]] == want_keys
        assert r.err_key == rk.err_key and r.act_dist == rk.act_dist
    assert (r.pkeys[:next_gidx] == U64(GUARD)).all() and (r.pkeys[next_gidx + total:] == U64(GUARD)).all()
    assert r.defer_flags == 0
    # the pinned head: what head_to_host copies, the rest untouched
    assert r.head[0] == r.err_key and r.head[1] == rk.chunk_base and r.head[2] == 0 and r.head[3] == 0
    assert r.head[4] == r.cand_total and r.head[5] == total and r.head[7] == 0 and r.head[9] == M64
    assert r.head[6] == GUARD and r.head[8] == GUARD


def picked_ranks(L):
    """Rank 0, the rank that receives fewest records and the one that receives most."""
    by = sorted(L.ranks, key=lambda rk: len(rk.recv))
    return {rk.rank: rk for rk in (L.ranks[0], by[0], by[-1])}.values()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_insert_of_a_real_level(oracle, world):
    """NP=2 level 22: a rank's own parents and what the other ranks send it,
    through k_claim, k_rec_claim, both settle passes, the fused overflow pass
    and scan, and the link emit: winners, links, parent keys, flags, table and
    counters are the model's."""
    L, _ = np2_level(oracle, world)
    seen = np2_seen(oracle)
    most = max(L.ranks, key=lambda rk: len(rk.recv))
    assert len(most.recv) > 256 and 0 < sum(most.isnew) < len(most.recv), "several record blocks, winners and losers"
    assert any(rec.fp in seen for rec in most.recv), "records of older levels' fingerprints"
    for rk in picked_ranks(L):
        assert rk.fr.n and rk.recv and rk.chunk_base > 0
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, world)
        check_insert(r, rk, L.spec)
        assert r.probes >= len(rk.recv)


def test_insert_paths_agree(oracle):
    """One rank's level down every spelling: the fused and the unfused overflow
    pass, tail 0 (k_shard_cand) and 1, the per-parent / per-record offsets from
    k_shard_scan_small and from the device scans, and the materialising emit
    on tile counts and on offsets: each is the model's, so all agree."""
    L, _ = np2_level(oracle, 3)
    seen = np2_seen(oracle)
    rk = L.ranks[2]
    assert rk.fr.n <= 1 << 16, "the fused pass is what ShardT would take here"
    cand = sum(len(cm.Parent(L.spec, x).succ) for x in rk.next)
    heads = []
    for kw in (dict(), dict(unfused=1), dict(tail=0), dict(unfused=1, tail=0), dict(next_gidx=77)):
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, 3, **kw)
        check_insert(r, rk, L.spec, next_gidx=kw.get("next_gidx", 0))
        heads.append(r.head)
    assert all(h == heads[0] for h in heads)
    for kw in (dict(path=0), dict(path=1), dict(path=2), dict(path=1, tail=0)):
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, 3, emit=0, **kw)
        check_insert(r, rk, L.spec, emit=0, path=kw["path"])
        assert r.cand_total == cand


def shaped(oracle):
    """Rank 1 of 3 on the first 300 of its parents of NP=2 level 22, and new
    fingerprints it owns: one with an own copy, one without."""
    L, _ = np2_level(oracle, 3)
    seen = np2_seen(oracle)
    base = L.ranks[1]
    fr = sm.sub_frontier(base.fr, range(300))
    plain = sm.settle_rank(L.spec, fr, [], seen, 1, 3)
    own = [(i, t) for i in range(fr.n) for t in range(32) if plain.newmask[i] >> t & 1]
    assert own
    i, t = own[len(own) // 2]
    far = next(rec for rec in base.recv if rec.fp not in seen and rec.fp not in {c[2] for c in fr.copies(True)})
    return L.spec, seen, fr, plain, (i, t), far


def shaped_run(spec, seen, fr, recv):
    rk = sm.settle_rank(spec, fr, recv, seen, 1, 3)
    r = run_insert(sm.K_INSERT, spec, rk, seen, 3)
    check_insert(r, rk, spec)
    return rk, r


def test_a_record_displaces_an_own_claim_and_the_other_way(oracle):
    spec, seen, fr, plain, (i, t), _ = shaped(oracle)
    a, x, _, fp = fr.parent(i).succ[t]
    # from rank 0: a smaller key than any of rank 1's own, so the record wins
    rk, r = shaped_run(spec, seen, fr, [sm.Record(sm.record_key(0, 5, 3, a), x, fp, a)])
    assert plain.newmask[i] >> t & 1 and not rk.newmask[i] >> t & 1 and rk.isnew == [1]
    assert int(r.flag[0]) == sm.RF_DISPLACER and not int(r.newmask[i]) >> t & 1
    assert r.level_new == plain.level_new and r.chunk_base == plain.chunk_base - 1
    # from rank 2: a larger key, the own claim stays
    rk, r = shaped_run(spec, seen, fr, [sm.Record(sm.record_key(2, 5, 3, a), x, fp, a)])
    assert rk.newmask == plain.newmask and rk.isnew == [0]
    # (k_claim's inserter stored its claim: the record finds the smaller claim and is out at once)
    assert int(r.flag[0]) in (sm.RF_OUT, sm.RF_CAND) and int(r.newmask[i]) >> t & 1


def test_two_senders_one_fingerprint_in_both_arrival_orders(oracle):
    spec, seen, fr, plain, _, far = shaped(oracle)
    lo = sm.Record(sm.record_key(0, 900, 2, far.action), far.tuple, far.fp, far.action)
    hi = sm.Record(sm.record_key(2, 1, 0, far.action), far.tuple, far.fp, far.action)
    got = []
    for recv in ([lo, hi], [hi, lo]):
        rk, r = shaped_run(spec, seen, fr, recv)
        j = recv.index(lo)
        assert rk.isnew[j] == 1 and rk.isnew[1 - j] == 0, "the smaller key wins wherever it stands"
        assert int(r.pkeys[r.level_new - 1]) == lo.key and int(r.link[r.level_new - 1]) == sm.LINK_REC | j
        got.append((r.entries, [int(m) for m in r.newmask], r.level_new))
    assert got[0] == got[1]


def test_a_record_of_an_older_levels_fingerprint_is_out(oracle):
    spec, seen, fr, plain, _, far = shaped(oracle)
    L, _ = np2_level(oracle, 3)
    old = next(rec for rec in L.ranks[1].recv if rec.fp in seen)
    rk, r = shaped_run(spec, seen, fr, [old, far])
    assert rk.isnew == [0, 1] and int(r.flag[0]) == sm.RF_OUT and int(r.flag[1]) == sm.RF_INSERTER
    assert r.entries[old.fp] == ~OLD & M64


@pytest.mark.parametrize("nrec", [255, 256, 257])
def test_insert_without_own_parents(oracle, nrec):
    """n_local = 0: k_win_scan's extra mark sits at cell 0; 255 / 256 / 257
    records: the record emit's ballots over a partial block, a full one, and a
    block of one record."""
    L, _ = np2_level(oracle, 3)
    seen = np2_seen(oracle)
    base = L.ranks[0]
    recv = base.recv[:nrec]
    assert len(recv) == nrec and 0 < sum(1 for rec in recv if rec.fp not in seen)
    rk = sm.settle_rank(L.spec, sm.sub_frontier(base.fr, []), recv, seen, 0, 3)
    assert rk.chunk_base == 0 and rk.level_new > 0
    for kw in (dict(), dict(unfused=1), dict(emit=0), dict(emit=0, path=1), dict(emit=0, path=2)):
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, 3, **kw)
        check_insert(r, rk, L.spec, emit=kw.get("emit", 1), path=kw.get("path", 0))


def test_insert_without_records(oracle):
    """records = 0: k_win_scan's extra mark is the total."""
    L, _ = np2_level(oracle, 3)
    seen = np2_seen(oracle)
    base = L.ranks[0]
    rk = sm.settle_rank(L.spec, base.fr, [], seen, 0, 3)
    assert rk.chunk_base == rk.level_new > 0
    for kw in (dict(), dict(unfused=1), dict(emit=0, path=1), dict(emit=0, path=2)):
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, 3, **kw)
        check_insert(r, rk, L.spec, emit=kw.get("emit", 1), path=kw.get("path", 0))


def test_an_invariant_violating_record_gives_the_error_key(fixtures):
    """The variant-1 NoLostUpdate violator arrives as a record: err_key is the
    record's key with the invariant kind in the low byte."""
    trace = fixtures["variant1_lost_update"]["trace"]
    cfg = kubecheck.ModelConfig(variant=1, invariants=7)
    spec = kubecheck.Spec(cfg)
    bad = np.array(trace[-1], dtype=U64)
    assert spec.check_invariants(bad) == "NoLostUpdate"
    prev = cm.Frontier(spec, np.array([trace[-2]], dtype=U64))
    act = next(s[0] for s in prev.parent(0).succ if s[1].tobytes() == bad.tobytes())
    fp = spec.fingerprint_own(bad)
    rank = cm.owner(fp, 2)
    key = sm.record_key(1 - rank, 4321, 6, act)
    rk = sm.settle_rank(spec, sm.sub_frontier(prev, []), [sm.Record(key, bad, fp, act)], set(), rank, 2)
    assert rk.err_key == (key & ~0xff) | cm.E_INVARIANT and rk.isnew == [1]
    for path in (0, 1):
        r = run_insert(sm.K_INSERT, spec, rk, set(), 2, emit=0, path=path)
        check_insert(r, rk, spec, emit=0, path=path)
        assert r.err_key == (key & ~0xff) | cm.E_INVARIANT


@pytest.mark.parametrize("world", [2, 3])
def test_tlc_order_keys_find_the_same_states(oracle, world):
    """TLC-order claim keys (G << 12 | position << 4 | rank), the rank-select
    map from gpos: the same set of new states as under rank-major keys, the
    winner of each the copy of smallest (G, position, rank)."""
    L, nxt = np2_level(oracle, world, tlc=True)
    P, _ = np2_level(oracle, world)
    seen = np2_seen(oracle)
    W = L.whole.n
    for rk, prk in zip(L.ranks, P.ranks):
        assert {x.tobytes() for x in rk.next} == {x.tobytes() for x in prk.next}
        r = run_insert(sm.K_INSERT, L.spec, rk, seen, world, tlc=True, W=W)
        check_insert(r, rk, L.spec, tlc=True)


# -------------------------------------------------------------------- emit links
def test_emit_links_wave_loop_and_capacity(oracle):
    """With nothing seen before, every distinct successor is new: a wave of 64
    parents has more than 64 winners and the r += 64 loop runs.  cap at the
    total, one below and 0: below the total DF_CAPACITY is set, nothing at or
    past cap is written, everything below is right, and a second launch with
    room gives the whole answer."""
    L, _ = np2_level(oracle, 2)
    base = L.ranks[0]
    fr = sm.sub_frontier(base.fr, range(600))
    rk = sm.settle_rank(L.spec, fr, base.recv[:300], set(), 0, 2)
    per_wave = [sum(popcounts(rk.newmask[k:k + 64])) for k in range(0, fr.n, 64)]
    assert max(per_wave) > 128, "a wave with more than two rounds of winners"
    total = rk.level_new
    assert total > rk.chunk_base > 0
    r = run_insert(sm.K_INSERT, L.spec, rk, set(), 2, cap=total)
    check_insert(r, rk, L.spec)
    for cap in (total - 1, rk.chunk_base, rk.chunk_base - 1, 0):
        r = run_insert(sm.K_INSERT, L.spec, rk, set(), 2, cap=cap)
        assert r.defer_flags == sm.DF_CAPACITY and r.head[7] == sm.DF_CAPACITY
        assert [int(x) for x in r.link[:cap]] == rk.link[:cap] and (r.link[cap:] == U64(GUARD)).all()
        assert [int(x) for x in r.pkeys[:cap]] == rk.pkeys[:cap] and (r.pkeys[cap:] == U64(GUARD)).all()
        assert r.level_new == total and r.head[5] == total
        r = run_insert(sm.K_INSERT, L.spec, rk, set(), 2, cap=cap, cap2=total)
        assert r.first_defer_flags == sm.DF_CAPACITY
        check_insert(r, rk, L.spec)


# ------------------------------------------------------------------ first-claim
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("compact", [0, 1])
def test_first_claim_insert(oracle, world, compact):
    """First-claim mode: a fingerprint this rank's k_claim inserted is old to
    every record; of the others exactly one record a fingerprint is new."""
    L, _ = np2_level(oracle, world)
    seen = np2_seen(oracle)
    spec = L.spec
    rk = max(L.ranks, key=lambda r: len(r.recv))
    n, nrec = rk.fr.n, len(rk.recv)
    own_fps = {fp for _, _, fp, _ in rk.fr.copies(True) if cm.owner(fp, world) == rk.rank}
    rec_only = {rec.fp for rec in rk.recv} - own_fps - seen
    assert rec_only and any(rec.fp in own_fps - seen for rec in rk.recv), "records new, and records an own copy beats"
    for emit in (1, 0):
        r = run_insert(sm.K_INSERT_FIRST, spec, rk, seen, world, path=compact, emit=emit)
        # own copies: one winner of every unseen owned fingerprint
        winners = {}
        for i, t, fp, _ in rk.fr.copies(True):
            if int(r.newmask[i]) >> t & 1:
                assert cm.owner(fp, world) == rk.rank
                winners[fp] = winners.get(fp, 0) + 1
        assert set(winners) == own_fps - seen and all(k == 1 for k in winners.values())
        # records: never one an own copy covers; one each of the rest
        rwin = {}
        for j, rec in enumerate(rk.recv):
            assert int(r.isnew[j]) in (0, 1)
            if int(r.isnew[j]):
                rwin[rec.fp] = rwin.get(rec.fp, 0) + 1
        assert set(rwin) == rec_only and all(k == 1 for k in rwin.values())
        own_new, rec_new = sum(winners.values()), sum(rwin.values())
        assert r.chunk_base == own_new and r.level_new == own_new + rec_new == len((own_fps | rec_only) - seen)
        assert r.level_new == rk.level_new
        assert set(r.entries) == set(r.pre) | own_fps | rec_only
        cells = r.tiles + r.rgrid
        wt = cm.tile_popcounts([int(m) for m in r.newmask]) + \
            [int(r.isnew[k:k + 256].sum()) for k in range(0, nrec, 256)]
        assert [int(x) for x in r.wtot[:cells]] == wt
        off, _ = sm.owner_offsets(wt, 1)
        assert [int(x) for x in r.woff[:cells]] == [int(x) for x in off] and int(r.woff[cells]) == r.level_new
        # both emits place every winner exactly once: own in (parent, position) order, records in receive order
        own_links = [i << 8 | t for i in range(n) for t in range(32) if int(r.newmask[i]) >> t & 1]
        rec_links = [sm.LINK_REC | j for j in range(nrec) if int(r.isnew[j])]
        states = [rk.fr.parent(lk >> 8).succ[lk & 0xff][1] for lk in own_links] + \
                 [rk.recv[lk ^ sm.LINK_REC].tuple for lk in rec_links]
        if emit:
            assert [int(x) for x in r.link[:r.level_new]] == own_links + rec_links
            assert (r.link[r.level_new:] == U64(GUARD)).all()
        else:
            want = [[int(w) for w in spec.pack(x)] for x in states]
            assert [[int(w) for w in s] for s in r.next[:r.level_new]] == want
            assert sum(r.act_dist) == r.level_new
        assert [int(x) & ~0xff for x in r.pkeys[own_new:r.level_new]] == \
            [rk.recv[lk ^ sm.LINK_REC].key & ~0xff for lk in rec_links]
        assert {x.tobytes() for x in states} == {x.tobytes() for x in rk.next}


# -------------------------------------------------------------------- TLC order
def check_tlc(pkeys, links, other):
    W = len(other)
    own, over = sm.tlc_words(pkeys, W)
    assert over == 0
    assert all(a & b == 0 for a, b in zip(own, other)), "one successor, two owners"
    wmask = [a | b for a, b in zip(own, other)]
    want = sm.tlc_order(pkeys, links, wmask)
    rc, r = sm.tlc(pkeys, links, other)
    assert rc == 0 and r.overflow == 0
    assert [int(x) for x in r.wmask] == wmask
    assert [int(x) for x in r.wbase] == want["wbase"]
    assert [int(x) for x in r.gnew] == want["gnew"]
    assert [int(x) for x in r.bits] == want["bits"]
    assert [int(x) for x in r.brank] == want["brank"]
    assert [int(x) for x in r.link] == want["link"]
    assert [int(x) for x in r.pkeys] == want["pkeys"]
    assert [int(x) for x in r.gpos] == want["gpos"]
    # a bijection onto [0, nn), sorted by G
    assert sorted(int(x) for x in r.link) == sorted(links) and want["gpos"] == sorted(set(want["gpos"]))
    return r, want


@pytest.mark.parametrize("W", [1, 32, 33])
def test_tlc_word_edges(W):
    """Positions 0 and 31 of a parent's word; new G values at bit 0 and bit 31
    of a bitmap word and in the next word; links distinct so the permutation
    shows."""
    rng = np.random.default_rng(W)
    pairs = [(g, t) for g in range(W) for t in range(32)]
    mine = [pairs[k] for k in sorted(rng.choice(len(pairs), size=min(len(pairs) // 3, 257), replace=False))]
    for must in ((0, 0), (0, 31), (W - 1, 0), (W - 1, 31)):
        if must not in mine:
            mine.append(must)
    rest = [p for p in pairs if p not in set(mine)]
    theirs = [rest[k] for k in rng.choice(len(rest), size=len(rest) // 2, replace=False)] if W > 1 else []
    order = list(rng.permutation(len(mine)))
    pkeys = [sm.record_key(3, mine[k][0], mine[k][1], 5) for k in order]
    links = [1000 + k for k in range(len(pkeys))]
    other = [0] * W
    for g, t in theirs:
        other[g] |= 1 << t
    own, _ = sm.tlc_words(pkeys, W)
    gn = set(sm.tlc_order(pkeys, links, [a | b for a, b in zip(own, other)])["gnew"])
    assert 0 in gn, "this rank's (G 0, position 0) is the level's first state"
    if W > 1:
        assert any(g & 31 == 31 for g in gn) and any(g & 31 == 0 for g in gn) and max(gn) >= 32
    check_tlc(pkeys, links, other)
    if W == 1:
        # every position of the one parent is this rank's: G = position, bits = one full word
        pk = [sm.record_key(0, 0, t) for t in range(32)]
        want = sm.tlc_order(pk, list(range(32)), [0xffffffff])
        assert want["gnew"] == list(range(32)) and want["bits"] == [0xffffffff, 0] and want["brank"] == [0, 32]
        check_tlc(pk, list(range(32)), [0])


@pytest.mark.parametrize("nn", [0, 257])
def test_tlc_sizes(nn):
    """No new state at this rank (the scans still run: wbase and brank are the
    other ranks' alone); 257 = one block and one thread."""
    W = 60
    pairs = [(g, t) for g in range(W) for t in range(0, 32, 3)]
    assert len(pairs) >= 2 * nn
    pkeys = [sm.record_key(1, g, t) for g, t in pairs[:nn]]
    other = [0] * W
    for g, t in pairs[nn:]:
        other[g] |= 1 << t
    r, want = check_tlc(pkeys, list(range(nn)), other)
    assert not r.bits.any() if nn == 0 else int(r.bits.sum()) > 0


def test_tlc_overflow_keys():
    """A parent G at or past the level's width and a position of 32 or more are
    counted, and k_tlc_mask writes nothing for them."""
    W = 5
    good = [sm.record_key(0, 4, 31), sm.record_key(0, 0, 0)]
    bad = [sm.record_key(0, W, 0), sm.record_key(0, 1, 32), sm.record_key(0, 0xffffffff, 255)]
    assert sm.tlc_words(good + bad, W) == ([1, 0, 0, 0, 1 << 31], 3)
    rc, r = sm.tlc(good + bad, list(range(5)), [0] * W)
    assert rc == 0 and r.overflow == 3
    assert [int(x) for x in r.wmask] == [1, 0, 0, 0, 1 << 31]
    for sec in (r.wbase, r.gnew, r.bits, r.brank, r.gpos):
        assert (sec == U64(GUARD32)).all()
    assert (r.link == U64(GUARD)).all() and (r.pkeys == U64(GUARD)).all()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_tlc_kernels_reproduce_the_oracles_order(oracle, world):
    """The model's TLC-order level of NP=2 level 22: each rank's parent keys
    through the kernels, the other ranks' words as the all-reduce would bring
    them; the states sorted by the kernels' G are the oracle's next level in
    its order."""
    L, nxt = np2_level(oracle, world, tlc=True)
    W = L.whole.n
    words = [sm.tlc_words(rk.pkeys, W)[0] for rk in L.ranks]
    by_g = {}
    for rk in L.ranks:
        assert rk.level_new > 0
        other = [0] * W
        for s, w in enumerate(words):
            if s != rk.rank:
                other = [a | b for a, b in zip(other, w)]
        r, want = check_tlc(rk.pkeys, rk.link, other)
        back = {lk: k for k, lk in enumerate(rk.link)}
        for g, lk in zip(r.gpos, r.link):
            assert int(g) not in by_g
            by_g[int(g)] = rk.next[back[int(lk)]].tobytes()
    assert [by_g[g] for g in range(len(nxt))] == [t.tobytes() for t in nxt]
