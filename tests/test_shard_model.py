"""shard_model.py against the oracle, and the host-side validation of
kc_shard_selftest (no GPU: bad input answers -EINVAL before any device is
looked for, good input -ENODEV on a machine without one).

The model of a sharded level is held to the oracle here so that the GPU tests
(test_gpu_shard_kernels.py) do not compare the kernels with a model that only
agrees with itself: at every world size the ranks' new states together are the
oracle's next level, under TLC order in the oracle's own (sequential-BFS)
order, and the links alone rebuild them."""
import errno

import numpy as np
import pytest

import claim_model as cm
import kubecheck
import shard_model as sm
from claim_model import M64

U64 = np.uint64
WORLDS = (1, 2, 3, 8, 15)
_cache = {}


def level_setup(oracle, np_, lv):
    """(spec, the level as a Frontier, the owner-projected fingerprints of
    levels 1 .. lv, the oracle's level lv + 1), once per level."""
    if (np_, lv) not in _cache:
        ocfg = oracle.config(np_=np_)
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=np_))
        seen = set()
        count = 0
        for k in range(1, lv + 1):
            for t in oracle.level_tuples(ocfg, k):
                seen.add(spec.fingerprint_own(t))
                count += 1
        assert len(seen) == count
        _cache[np_, lv] = (spec, cm.Frontier(spec, oracle.level_tuples(ocfg, lv)), seen,
                           oracle.level_tuples(ocfg, lv + 1))
    return _cache[np_, lv]


LEVELS = [(2, 22), (1, 30)]


@pytest.mark.parametrize("np_,lv", LEVELS)
@pytest.mark.parametrize("world", WORLDS)
def test_ranks_together_find_the_oracles_next_level(oracle, np_, lv, world):
    spec, whole, seen, nxt = level_setup(oracle, np_, lv)
    assert whole.n > 256 and len(nxt) > 0
    L = sm.Level(spec, None, seen, world, whole=whole)
    assert sorted(g for rk in L.ranks for g in rk.G) == list(range(whole.n))
    new = [x.tobytes() for rk in L.ranks for x in rk.next]
    assert len(new) == len(set(new)), "a state new at two ranks, or twice at one"
    assert set(new) == {t.tobytes() for t in nxt}
    assert sum(rk.level_new for rk in L.ranks) == len(nxt)
    for rk in L.ranks:
        # a new state lives where its fingerprint does; own winners come first
        assert all(cm.owner(spec.fingerprint_own(x), world) == rk.rank for x in rk.next)
        assert rk.chunk_base == sum(cm.popcount(m) for m in rk.newmask)
        assert rk.level_new - rk.chunk_base == sum(rk.isnew)
        assert all(lk & sm.LINK_REC for lk in rk.link[rk.chunk_base:])
        assert not any(lk & sm.LINK_REC for lk in rk.link[:rk.chunk_base])
        assert sum(rk.act_dist) == rk.level_new and rk.err_key == M64
        # what is sent is what is received, owner by owner
        assert sum(sum(row) for row in rk.tcnt) == sum(len(g) for g in rk.send)
        assert [len(g) for g in rk.send] == [sum(row) for row in rk.tcnt]
        assert len(rk.recv) == sum(len(s.send[rk.rank]) for s in L.ranks)
        # the links alone give the states back
        assert [x.tobytes() for x in L.rebuild(rk)] == [x.tobytes() for x in rk.next]
    if world == 1:
        assert not L.ranks[0].recv and L.ranks[0].chunk_base == len(nxt)


@pytest.mark.parametrize("np_,lv", LEVELS)
@pytest.mark.parametrize("world", WORLDS)
def test_tlc_order_is_the_oracles_order(oracle, np_, lv, world):
    """Under TLC-order keys the winners are the first discoverers of a
    sequential BFS, and the renumbering puts them in its order."""
    spec, whole, seen, nxt = level_setup(oracle, np_, lv)
    L = sm.Level(spec, None, seen, world, tlc=True, whole=whole)
    W = whole.n
    words = [sm.tlc_words(rk.pkeys, W) for rk in L.ranks]
    assert all(over == 0 for _, over in words)
    wmask = [0] * W
    for w, _ in words:
        assert all(a & b == 0 for a, b in zip(wmask, w)), "one successor, two owners"
        wmask = [a | b for a, b in zip(wmask, w)]
    by_g = {}
    for rk in L.ranks:
        r = sm.tlc_order(rk.pkeys, rk.link, wmask)
        assert r["gpos"] == sorted(r["gpos"])
        for g, i in zip(r["gpos"], r["order"]):
            assert g not in by_g
            by_g[g] = rk.next[i].tobytes()
    assert sorted(by_g) == list(range(len(nxt)))
    assert [by_g[g] for g in range(len(nxt))] == [t.tobytes() for t in nxt]


def test_rank_major_and_tlc_keys_find_the_same_states(oracle):
    spec, whole, seen, nxt = level_setup(oracle, 2, 22)
    a = sm.Level(spec, None, seen, 3, whole=whole)
    b = sm.Level(spec, None, seen, 3, tlc=True, whole=whole)
    for ra, rb in zip(a.ranks, b.ranks):
        assert {x.tobytes() for x in ra.next} == {x.tobytes() for x in rb.next}
    assert any(ra.link != rb.link for ra, rb in zip(a.ranks, b.ranks)), "the two orders never pick another copy"


def test_keys():
    k = sm.record_key(14, 0xfffffffe, 31, 21)
    assert sm.key_fields(k) == (14, 0xfffffffe, 31, 21)
    assert sm.claim_key(k, False) == 14 << 40 | 0xfffffffe << 8 | 31
    assert sm.claim_key(k, True) == 0xfffffffe << 12 | 31 << 4 | 14
    # rank-major: the rank decides first; TLC order: the parent's G, then the position, then the rank
    assert sm.claim_key(sm.record_key(1, 0, 0), False) > sm.claim_key(sm.record_key(0, 9, 9), False)
    assert sm.claim_key(sm.record_key(1, 0, 0), True) < sm.claim_key(sm.record_key(0, 0, 1), True)


def test_owner_offsets_row_and_send_buffer():
    off, tot = sm.owner_offsets([1, 0, 2, 0, 0, 0, 3, 4, 0], 3)
    assert list(off) == [0, 1, 1, 3, 3, 3, 3, 6, 10] and tot == [3, 0, 7]
    head = dict(defer_err=M64, overflow=0, batch_used=0)
    assert sm.owner_row(tot, 3, head, 5, 77, 0, M64) == [3, 0, 7, 5, 77, 0]
    assert sm.owner_row(tot, 3, dict(head, defer_err=76), 5, 77, 0, M64)[4] == 76
    assert sm.owner_row(tot, 3, dict(head, defer_err=78), 5, 77, 0, M64)[4] == 77
    assert sm.owner_row(tot, 3, dict(head, defer_err=1), 5, 77, 1, 0x12)[4] == 0x12
    assert sm.owner_row(tot, 3, dict(head, defer_err=1), 5, 77, 0, 0x12)[4] == 1
    assert sm.owner_row(tot, 3, dict(head, batch_used=2), 5, 77, 0, M64)[5] == 1
    # two tiles, two owners, one word a record: tile 0 staged [a0 b0 b1], tile 1 [a1]
    buf = sm.send_buffer([10, 20, 21, 11], [0, 3], [[1, 1], [2, 0]], 2, 1)
    assert buf == [10, 11, 20, 21]
    assert sm.send_buffer([10, 20, 21, 11], [0, M64], [[1, 1], [2, 0]], 2, 1) == [10, None, 20, 21]


# ------------------------------------------------------------------ validation
EINVAL = -errno.EINVAL


def ok():
    return {0, -errno.ENODEV} if kubecheck.device_count() else {-errno.ENODEV}


def test_owner_scan_validates_on_the_host():
    cells = [1, 2, 3, 4, 5, 6]
    assert sm.owner_scan(0, 3, 2, cells)[0] in ok()
    assert sm.owner_scan(2, 3, 0, [])[0] in ok()
    assert sm.owner_scan(4, 3, 2, cells)[0] == EINVAL                      # mode
    assert sm.owner_scan(0, 0, 2, [])[0] == EINVAL                         # world 0
    assert sm.owner_scan(0, 16, 1, [0] * 16)[0] == EINVAL                  # world 16
    assert sm.owner_scan(0, 3, 0, [])[0] == EINVAL                         # no cells in a tile scan
    assert sm.owner_scan(0, 3, 2, cells[:5])[0] == EINVAL                  # a short matrix
    assert sm.owner_scan(0, 3, 2, [1 << 32] + cells[1:])[0] == EINVAL      # a cell over 32 bits
    assert sm.owner_scan(0, 2, 2, [M64 >> 32] * 4)[0] == EINVAL            # the total over 32 bits
    assert sm.owner_scan(2, 3, 2, [256] + cells[1:])[0] == EINVAL          # a cell over 8 bits
    assert sm.owner_scan(2, 2, 8193, [0] * 16386)[0] == EINVAL             # past OWNER_SMALL_SCAN
    assert sm.owner_scan(3, 2, 8193, [0] * 16386)[0] in ok()
    assert sm.owner_scan(0, 3, 2, cells, level1=2)[0] == EINVAL
    assert sm.owner_scan(0, 3, 2, cells, want_row=2)[0] == EINVAL
    assert sm.owner_scan(0, 3, 2, cells, off_len=7)[0] == EINVAL           # off: 8 cells (two 16-B groups)
    assert sm.owner_scan(0, 3, 2, cells, aft=1 << 11)[0] == EINVAL
    assert b"kc_shard_selftest" in kubecheck.load().kc_last_error()


def gather_case():
    cfg = kubecheck.ModelConfig(np=2)
    tcnt = [1, 1, 2, 0]                                  # [owner][tile]
    return cfg, dict(world=2, T=2, chunked=0, stage=list(range(4 * 6)), stoff=[0, 3], tcnt_flat=tcnt,
                     offs=[0, 1, 2, 4])


def test_gather_validates_on_the_host():
    cfg, kw = gather_case()
    assert sm.gather(cfg, **kw)[0] in ok()
    assert sm.gather(cfg, **dict(kw, chunked=1, offs=[0, 2]))[0] in ok()
    assert sm.gather(cfg, **dict(kw, stoff=[0, M64]))[0] in ok()
    assert sm.gather(kubecheck.ModelConfig(np=3), **kw)[0] == EINVAL       # no such record width here
    assert sm.gather(cfg, **dict(kw, world=16))[0] == EINVAL
    assert sm.gather(cfg, **dict(kw, chunked=2))[0] == EINVAL
    assert sm.gather(cfg, **dict(kw, offs=[0, 1, 2, 3]))[0] == EINVAL      # not the exclusive sums
    assert sm.gather(cfg, **dict(kw, chunked=1, offs=[0, 1]))[0] == EINVAL  # not the chunk sums'
    assert sm.gather(cfg, **dict(kw, offs=[0, 1, 2]))[0] == EINVAL         # a short offset matrix
    assert sm.gather(cfg, **dict(kw, stoff=[0, 4]))[0] == EINVAL           # a segment past the staging buffer
    assert sm.gather(cfg, **dict(kw, stoff=[2, 3]))[0] == EINVAL           # ... ending past it
    assert sm.gather(cfg, **dict(kw, stage=list(range(23))), nstage=4)[0] == EINVAL   # not whole records
    assert sm.gather(cfg, **kw, out_records=3)[0] == EINVAL                # the send buffer is sized exactly
    assert sm.gather(cfg, **kw, out_records=5)[0] == EINVAL


def small_frontier(oracle):
    cfg = kubecheck.ModelConfig(np=1)
    spec = kubecheck.Spec(cfg)
    return cfg, spec, cm.Frontier(spec, oracle.level_tuples(oracle.config(), 12))


def test_pack_validates_on_the_host(oracle):
    cfg, spec, fr = small_frontier(oracle)
    n, packed = fr.n, fr.packed()
    full = [(1 << len(fr.parent(i).succ)) - 1 for i in range(n)]
    assert sm.pack(cfg, packed, n, full, 3, 1)[0] in ok()
    assert sm.pack(cfg, packed, n, full, 3, 1, gpos=list(range(n)))[0] in ok()
    assert sm.pack(cfg, packed, n, [0] * n, 3, 1)[0] in ok()                            # nothing marked
    assert sm.pack(cfg, packed, n, full, 3, 3)[0] == EINVAL                             # rank >= world
    assert sm.pack(cfg, packed, n, full, 16, 1)[0] == EINVAL
    assert sm.pack(cfg, packed, n, [full[0] << 1] + full[1:], 3, 1,
                   total=sum(cm.popcount(m) for m in full))[0] == EINVAL                # a bit past the successors
    assert sm.pack(cfg, packed, n, full, 3, 1, total=1)[0] == EINVAL                    # the send buffer's size
    assert sm.pack(cfg, packed, n, full, 3, 1, gpos=[1 << 32] + [0] * (n - 1))[0] == EINVAL
    assert sm.pack(cfg, packed, n, full[:-1], 3, 1)[0] == EINVAL                        # a short repmask
    bad = packed.copy()
    bad[1] = M64
    assert sm.pack(cfg, bad, n, full, 3, 1)[0] == EINVAL                                # an out-of-domain parent


def test_materialize_and_undo_validate_on_the_host(oracle):
    cfg, spec, fr = small_frontier(oracle)
    n, packed = fr.n, fr.packed()
    a, x, _, _ = fr.parent(0).succ[0]
    row = [int(w) for w in spec.pack(x)] + [sm.record_key(1, 5, 0, a)]
    links = [0 << 8 | 0, sm.LINK_REC | 0, (n - 1) << 8 | 0]
    assert len(fr.parent(n - 1).succ) > 0
    assert sm.materialize(cfg, packed, n, links, [row])[0] in ok()
    assert sm.materialize(cfg, packed, n, links, [row], prev_gpos=list(range(n)), prev_counts=0)[0] in ok()
    assert sm.materialize(cfg, packed, n, [n << 8], [row])[0] == EINVAL                 # a parent past nprev
    assert sm.materialize(cfg, packed, n, [len(fr.parent(0).succ)], [row])[0] == EINVAL  # a position past the count
    assert sm.materialize(cfg, packed, n, [sm.LINK_REC | 1], [row])[0] == EINVAL        # a record past nrec
    assert sm.materialize(cfg, packed, n, [sm.LINK_REC | 0], [])[0] == EINVAL           # ... with no records
    assert sm.materialize(cfg, packed, n, [], [row])[0] == EINVAL                       # no states
    assert sm.materialize(cfg, packed, n, links, [[M64] + row[1:]])[0] == EINVAL        # a record outside the domain
    assert sm.materialize(cfg, packed, n, links, [row], rank=15)[0] == EINVAL
    assert sm.materialize(cfg, packed, n, links, [row], prev_gpos=[1 << 32] * n)[0] == EINVAL
    assert sm.materialize(cfg, packed, n, links, [row], prev_counts=2)[0] == EINVAL
    assert sm.undo(cfg, packed, n, [0] * cm.NACT)[0] in ok()
    assert sm.undo(cfg, packed, n, [0] * (cm.NACT - 1))[0] == EINVAL
    assert sm.undo(cfg, packed, n + 1, [0] * cm.NACT)[0] == EINVAL
    bad = packed.copy()
    bad[1] = M64
    assert sm.undo(cfg, bad, n, [0] * cm.NACT)[0] == EINVAL


def test_insert_validates_on_the_host(oracle):
    cfg, spec, fr = small_frontier(oracle)
    n = fr.n
    a, x, _, fpo = fr.parent(0).succ[0]
    rank = cm.owner(fpo, 3)
    other = (rank + 1) % 3
    rec = sm.Record(sm.record_key(other, 5, 0, a), x, fpo, a)
    rows = sm.record_rows(spec, [rec])
    nslots = 2 * (fr.total() + 2)
    kw = dict(level=13, nslots=nslots, world=3, rank=rank)

    def run(kind=sm.K_INSERT, f=fr, r=rows, **over):
        return sm.insert(kind, cfg, f, r, **{**kw, **over})[0]

    assert run() in ok()
    assert run(f=None) in ok()                                             # no own parents
    assert run(r=[]) in ok()                                               # no records
    assert run(emit=0, path=1) in ok() and run(emit=0, path=2) in ok() and run(unfused=1, tail=0) in ok()
    assert run(gpos=list(range(0, 2 * n, 2)), W=2 * n) in ok()
    assert run(sm.K_INSERT_FIRST) in ok() and run(sm.K_INSERT_FIRST, path=1, emit=0) in ok()
    assert run(f=None, r=[]) == EINVAL                                     # nothing at all
    assert run(world=1, rank=0) == EINVAL and run(world=16) == EINVAL and run(rank=3) == EINVAL
    assert run(level=0) == EINVAL
    assert run(path=3) == EINVAL and run(sm.K_INSERT_FIRST, path=2) == EINVAL
    assert run(path=1) == EINVAL                                           # links need the tile counts
    assert run(unfused=1, path=1, emit=0) == EINVAL
    assert run(gpos=list(range(n)), W=n, emit=0) == EINVAL                 # TLC order needs links
    assert run(sm.K_INSERT_FIRST, gpos=list(range(n)), W=n) == EINVAL      # ... and the deterministic mode
    assert run(gpos=list(range(n)), W=n - 1) == EINVAL                     # a G at W
    assert run(gpos=[0] * n, W=n) == EINVAL                                # gpos not increasing
    assert run(gpos=list(range(n)), W=0) == EINVAL
    def keyed(sender, parent):
        return sm.record_rows(spec, [sm.Record(sm.record_key(sender, parent, 0, a), x, fpo, a)])

    assert run(gpos=list(range(n)), W=n, r=keyed(other, n)) == EINVAL      # a record's G at W
    assert run(r=keyed(rank, 5)) == EINVAL                                 # the rank's own record
    assert run(r=keyed(3, 5)) == EINVAL                                    # a sender at world
    assert run(r=[[M64] + rows[0][1:]]) == EINVAL                          # a record outside the domain
    assert run(nslots=fr.total() + 1) == EINVAL                            # no room for the record and a free slot
    assert run(nslots=fr.total() + 2) in ok()
    assert run(sm.K_INSERT_FIRST, path=1, nslots=nslots + 1) == EINVAL     # odd compact table
    stray = np.zeros(2 * nslots, dtype=U64)
    stray[5] = 1
    assert run(table=stray) == EINVAL                                      # a claim word, no fingerprint
    far = np.zeros(2 * nslots, dtype=U64)
    far[0], far[1] = 12345, ~cm.make_claim(13, (32 * (n // 32 + 1)) << 12) & M64
    assert run(gpos=list(range(n)), W=n, table=far) == EINVAL              # a same-level claim's G past the bitmap
    assert run(gpos=list(range(n)), W=n, table=far, level=14) in ok()      # ... of another level: not looked at
    assert run(table=np.zeros(2 * nslots - 1, dtype=U64)) == EINVAL        # a short image
    assert run(next_gidx=(1 << 20) + 1) == EINVAL and run(tail=2) == EINVAL and run(aft=1 << 11) == EINVAL


def test_tlc_validates_on_the_host():
    pk = [sm.record_key(0, 1, 0), sm.record_key(0, 1, 31), sm.record_key(0, 0, 5)]
    lk = [0, 1, 2]
    assert sm.tlc(pk, lk, [0, 0])[0] in ok()
    assert sm.tlc([], [], [0, 0])[0] in ok()
    assert sm.tlc(pk + [sm.record_key(0, 2, 0)], lk + [3], [0, 0])[0] in ok()   # G = W: counted, not refused
    assert sm.tlc(pk, lk, [])[0] == EINVAL                                 # an empty level
    assert sm.tlc(pk, lk[:2], [0, 0])[0] == EINVAL                         # links short of keys
    assert sm.tlc(pk, lk, [0, 1 << 32])[0] == EINVAL                       # a position word over 32 bits
    assert sm.tlc(pk, lk, [0, 0], W=3)[0] == EINVAL                        # other[] short of W
    assert sm.tlc(pk, lk, [0, 0], nn=2)[0] == EINVAL                       # nn short of the keys
    lib = kubecheck.load()
    assert lib.kc_shard_selftest(99, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0) == EINVAL
    assert lib.kc_shard_selftest(1, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0) == EINVAL   # no cfg
