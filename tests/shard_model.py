"""Host model of one sharded BFS level (csrc/shard_kernels.h), and
the binding of kc_shard_selftest (csrc/shard_selftest.hip).  Helper module, no
tests here.  Plain Python over kubecheck.Spec, on claim_model's pieces.

Nothing of the kernels' structure is in the model: no scans, no ballots, no
wave prefixes.  A level is a frontier in sequential-BFS order (state g has
G = g); rank r holds the states whose owner-projected fingerprint it owns, in
G order.

  keys      a record's key is sender << 60 | parent << 16 | position << 8 |
            action (parent = the sender's local index, or its G under TLC
            order); its claim key is (sender, parent, position) packed as
            sender << 40 | parent << 8 | position, or under TLC order
            G << 12 | position << 4 | sender.
  send      per rank, the tile representatives of the fingerprints other ranks
            own (claim_model.representatives), grouped by owner, each group in
            tile order, then (parent, position) order.
  receive   the groups for one owner, concatenated in sender order.
  winners   of every fingerprint a rank owns that no earlier level holds, the
            copy with the smallest claim key among the rank's own copies and
            the records that reach it.
  emit      the rank's own winners in (parent, position) order (link parent <<
            8 | position), then the records' in receive order (link bit 63 |
            record index); the parent key is the record's key, or for an own
            winner rank << 60 | parent << 16 | position << 8.
  TLC order the next level's G of a new state = the new states of smaller
            (parent G, position); a rank's new states are put in G order.
  rebuild   a state from its link: the parent's successor at the position, or
            the state a record of the previous level's receive buffer carries.

The owner scans and the gather are modelled on counts alone: offsets are one
cumulative sum over the owner-major cells, the send buffer is the segments of
the staging buffer in (owner, tile) order."""
import ctypes as C

import numpy as np

import claim_model as cm
import kubecheck
from claim_model import FORE, M64, NACT, TILE, owner

CSUM_TILES = cm.CSUM_TILES
OWNER_SMALL_SCAN = 16384
GUARD, GUARD32 = cm.GUARD, cm.GUARD32
LINK_REC = 1 << 63
RW = {1: 4, 2: 6}              # Record<M>::RW (csrc/record.h): u64 words of a record at np 1, 2
HEAD_WORDS = ("err_key", "chunk_base", "overflow", "batch_used", "cand_total", "level_new", "emit_done",
              "defer_flags", "defer_inv_n", "defer_err")
HEAD_COPIED = (0, 1, 2, 3, 4, 5, 7, 9)     # the words head_to_host copies, each to the same index


# ------------------------------------------------------------------------- keys
def record_key(rank, parent, pos, action=0):
    return rank << 60 | parent << 16 | pos << 8 | action


def key_fields(key):
    """-> (rank, parent, position, low byte)"""
    return key >> 60, (key >> 16) & cm.M32, (key >> 8) & 0xff, key & 0xff


def claim_key(key, tlc):
    r, p, t, _ = key_fields(key)
    return p << 12 | t << 4 | r if tlc else r << cm.RANK_SHIFT | p << 8 | t


# ------------------------------------------------------------------------ level
class Record:
    __slots__ = ("key", "tuple", "fp", "action")

    def __init__(self, key, tup, fp, action):
        self.key, self.tuple, self.fp, self.action = key, tup, fp, action


class Rank:
    """What one rank holds, sends, receives and emits in a level."""


class Level:
    """One sharded level: `tuples` = the frontier in sequential-BFS order,
    `seen` = the owner-projected fingerprints of every earlier level and this
    one (the preload), over `world` ranks, with rank-major or TLC-order keys."""

    def __init__(self, spec, tuples, seen, world, tlc=False, whole=None):
        self.spec, self.world, self.tlc = spec, world, tlc
        whole = whole or cm.Frontier(spec, tuples)
        self.whole = whole
        fps = [spec.fingerprint_own(whole.parent(g).tuple) for g in range(whole.n)]
        self.ranks = []
        for r in range(world):
            rk = Rank()
            rk.rank = r
            rk.G = [g for g in range(whole.n) if owner(fps[g], world) == r]      # local index -> G
            rk.fr = sub_frontier(whole, rk.G)
            self.ranks.append(rk)
        for rk in self.ranks:
            self._send(rk)
        for rk in self.ranks:
            rk.recv = [rec for s in self.ranks for rec in s.send[rk.rank]]
            self._settle(rk, seen)

    def _pidx(self, rk, i):
        return rk.G[i] if self.tlc else i

    def _send(self, rk):
        reps, _ = cm.representatives(rk.fr, rk.rank, self.world)
        rk.reps = reps
        rk.tcnt = [[sum(1 for e in tile if e[3] == o) for tile in reps] for o in range(self.world)]
        rk.send = [[] for _ in range(self.world)]
        for tile in reps:
            for i, t, a, o in tile:                       # sorted: (parent, position) order
                _, x, _, fpo = rk.fr.parent(i).succ[t]
                rk.send[o].append(Record(record_key(rk.rank, self._pidx(rk, i), t, a), x, fpo, a))
        assert not rk.send[rk.rank]

    def _settle(self, rk, seen):
        best = {}                                           # fp -> (claim key, None | record index, i, t)
        for i, t, fp, _ in rk.fr.copies(True):
            if owner(fp, self.world) != rk.rank or fp in seen:
                continue
            c = claim_key(record_key(rk.rank, self._pidx(rk, i), t), self.tlc)
            if fp not in best or c < best[fp][0]:
                best[fp] = (c, None, i, t)
        for j, rec in enumerate(rk.recv):
            assert owner(rec.fp, self.world) == rk.rank
            if rec.fp in seen:
                continue
            c = claim_key(rec.key, self.tlc)
            if rec.fp not in best or c < best[rec.fp][0]:
                best[rec.fp] = (c, j, None, None)
        rk.claims = {fp: v[0] for fp, v in best.items()}    # the level's claim key of every new fingerprint
        rk.newmask = [0] * rk.fr.n
        rk.isnew = [0] * len(rk.recv)
        for c, j, i, t in best.values():
            if j is None:
                rk.newmask[i] |= 1 << t
            else:
                rk.isnew[j] = 1
        rk.link, rk.pkeys, rk.next, rk.act_dist = [], [], [], [0] * NACT
        rk.err_key = M64
        for i in range(rk.fr.n):
            for t in range(32):
                if rk.newmask[i] >> t & 1:
                    a, x, _, _ = rk.fr.parent(i).succ[t]
                    self._emit(rk, i << 8 | t, record_key(rk.rank, self._pidx(rk, i), t), x, a)
        rk.chunk_base = len(rk.link)
        for j, rec in enumerate(rk.recv):
            if rk.isnew[j]:
                self._emit(rk, LINK_REC | j, rec.key, rec.tuple, rec.action)
        rk.level_new = len(rk.link)

    def _emit(self, rk, link, key, x, action):
        rk.link.append(link)
        rk.pkeys.append(key)
        rk.next.append(x)
        rk.act_dist[action] += 1
        if self.spec.check_invariants(x) is not None:
            rk.err_key = min(rk.err_key, (key & ~0xff) | cm.E_INVARIANT)

    def rebuild(self, rk):
        """The rank's next states from its links alone."""
        out = []
        for lk in rk.link:
            out.append(rk.recv[lk ^ LINK_REC].tuple if lk & LINK_REC else rk.fr.parent(lk >> 8).succ[lk & 0xff][1])
        return out


def settle_rank(spec, fr, recv, seen, rank, world, tlc=False, G=None):
    """One rank's winners and emit for own parents `fr` (local index i has
    G[i]) and received records `recv` of any making (each owned by the rank)."""
    lv = Level.__new__(Level)
    lv.spec, lv.world, lv.tlc = spec, world, tlc
    rk = Rank()
    rk.rank, rk.fr, rk.recv = rank, fr, list(recv)
    rk.G = list(range(fr.n)) if G is None else list(G)
    lv._settle(rk, seen)
    return rk


def record_rows(spec, recs):
    """Records as the harness takes them: state words, then the key."""
    return [[int(w) for w in spec.pack(r.tuple)] + [r.key] for r in recs]


def sub_frontier(fr, index):
    sub = cm.Frontier.__new__(cm.Frontier)
    sub.spec, sub.block, sub.index = fr.spec, fr.block, [fr.index[k] for k in index]
    sub.n, sub.tiles = len(sub.index), (len(sub.index) + TILE - 1) // TILE
    return sub


# -------------------------------------------------------------------- TLC order
def tlc_words(pkeys, W):
    """k_tlc_mask: the position word of each parent G, and the keys outside the level."""
    w, over = [0] * W, 0
    for k in pkeys:
        _, g, t, _ = key_fields(k)
        if g >= W or t >= 32:
            over += 1
        else:
            w[g] |= 1 << t
    return w, over


def tlc_order(pkeys, links, wmask):
    """The renumbering of one rank's new states given the level's combined
    position words -> dict(wbase, gnew, bits, brank, link, pkeys, gpos)."""
    W = len(wmask)
    wbase = [0] * W
    for g in range(1, W):
        wbase[g] = wbase[g - 1] + cm.popcount(wmask[g - 1])
    gnew = []
    for k in pkeys:
        _, g, t, _ = key_fields(k)
        gnew.append(wbase[g] + cm.popcount(wmask[g] & ((1 << t) - 1)))
    bits = [0] * (W + 1)
    for gn in gnew:
        bits[gn >> 5] |= 1 << (gn & 31)
    brank = [0] * (W + 1)
    for w in range(1, W + 1):
        brank[w] = brank[w - 1] + cm.popcount(bits[w - 1])
    order = sorted(range(len(gnew)), key=lambda i: gnew[i])
    return dict(wbase=wbase, gnew=gnew, bits=bits, brank=brank, link=[links[i] for i in order],
                pkeys=[pkeys[i] for i in order], gpos=[gnew[i] for i in order], order=order)


# ------------------------------------------------------ owner scans and the gather
def owner_offsets(cells, world):
    """cells: the owner-major count matrix, flat -> (exclusive offsets, owner totals)."""
    c = np.asarray(cells, dtype=np.int64)
    off = np.cumsum(c) - c
    per = len(c) // world if world else 0
    return off, [int(c[o * per:(o + 1) * per].sum()) for o in range(world)]


def owner_row(totals, world, head, status_new, status_err, level1, init_err):
    """row[world + 3] as owner_row writes it; head: dict of the Counters' words."""
    se = min(status_err, head["defer_err"])
    if level1 and init_err != M64:
        se = init_err
    return list(totals) + [status_new, se, 1 if head["overflow"] or head["batch_used"] else 0]


def send_buffer(stage, stoff, tcnt, world, rw):
    """The gather: tcnt[o][tile], stoff[tile] (M64: nothing staged), stage =
    flat record words -> the send buffer's words, None where nothing is written."""
    T = len(stoff)
    out = []
    for o in range(world):
        for t in range(T):
            n = tcnt[o][t]
            if stoff[t] == M64:
                out += [None] * (n * rw)
                continue
            src = stoff[t] + sum(tcnt[k][t] for k in range(o))
            out += [int(x) for x in stage[src * rw:(src + n) * rw]]
    return out


# ----------------------------------------------------------------------- harness
class Result:
    pass


def _call(kind, cfg, par, a, b, need, guards, nres, aft, table=None):
    lib = kubecheck.load()
    at = [0]
    for k in need:
        at.append(at[-1] + FORE + k + aft)
    out = np.zeros(at[-1], dtype=np.uint64)
    for k, g in enumerate(guards):
        out[at[k]:at[k + 1]] = g
    res = np.full(nres, GUARD, dtype=np.uint64)
    par = np.array([int(x) & M64 for x in par], dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))   # noqa: E731
    c = (cfg or kubecheck.ModelConfig()).to_c()
    assert table is None or (table.dtype == np.uint64 and table.flags.c_contiguous)
    rc = lib.kc_shard_selftest(kind, C.byref(c), p(par), len(par), p(a), len(a), p(b), len(b),
                               None if table is None else p(table), 0 if table is None else len(table), p(out),
                               len(out), p(res), len(res))
    secs = []
    if rc == 0:
        for k, g in enumerate(guards):
            sec = out[at[k]:at[k + 1]]
            assert (sec[:FORE] == np.uint64(g)).all(), (k, "fore guard")
            assert (sec[FORE + need[k]:] == np.uint64(g)).all(), (k, "aft guard")
            secs.append(sec[FORE:FORE + need[k]].copy())
    return rc, secs, res


def owner_scan(mode, world, T, cells, head=None, status_new=0, status_err=M64, level1=0, init_err=M64, want_row=1,
               aft=8, off_len=None):
    """kind 0 -> (rc, Result: off, tot, host_tot, host_head, row, cells_after).
    Sections start as guards, so an untouched cell reads GUARD32 / GUARD."""
    head = dict(head or {})
    hw = [head.get(k, M64 if k in ("err_key", "defer_err") else 0) for k in HEAD_WORDS]
    ncell = world * T
    if off_len is None:
        off_len = max(4 * ((ncell + 3) // 4), ncell + 1) if mode < 2 else ncell
    rc, s, res = _call(0, None, [mode, world, T, status_new, status_err, level1, init_err, want_row, aft], cells, hw,
                       [off_len, 16, 16, 10, world + 3], [GUARD32, GUARD, GUARD, GUARD, GUARD], len(cells), aft)
    r = Result()
    if rc == 0:
        r.off, r.tot, r.host_tot, r.host_head, r.row = s
        r.cells_after = res
    return rc, r


def gather(cfg, world, T, chunked, stage, stoff, tcnt_flat, offs, nstage=None, aft=8, out_records=None):
    """kind 1 -> (rc, the send buffer's words); untouched words read GUARD."""
    rw = RW.get(cfg.np, 6)       # (another np: the harness refuses the config)
    nstage = len(stage) // rw if nstage is None else nstage
    total = int(sum(tcnt_flat)) if out_records is None else out_records
    b = np.concatenate([np.asarray(x, dtype=np.uint64) for x in (stoff, tcnt_flat, offs)])
    rc, s, _ = _call(1, cfg, [world, T, chunked, nstage, aft], stage, b, [total * rw], [GUARD], 0, aft)
    return rc, (s[0] if rc == 0 else None)


def pack(cfg, packed, n, repmask, world, rank, gpos=None, total=None, aft=8):
    """kind 3 -> (rc, Result: raw send buffer words, records as rows of state
    words + key, per_owner).  total: the marked successors (what sizes out)."""
    W = kubecheck.Spec(cfg).state_words
    total = sum(cm.popcount(m) for m in repmask) if total is None else total
    b = list(repmask) + (list(gpos) if gpos is not None else [])
    rc, s, res = _call(3, cfg, [n, world, rank, int(gpos is not None), aft], packed, b,
                       [total * RW.get(cfg.np, 6), total * (W + 1)], [GUARD, GUARD], world, aft)
    r = Result()
    if rc == 0:
        r.raw, r.records, r.per_owner = s[0], s[1].reshape(-1, W + 1), [int(x) for x in res]
    return rc, r


def materialize(cfg, prev_packed, nprev, links, records, rank=0, prev_gpos=None, prev_counts=1, n=None, nrec=None,
                aft=8):
    """kind 4: records = rows of state words + key -> (rc, Result: states[n][W],
    defer_err, next_cand, act_dist)."""
    W = kubecheck.Spec(cfg).state_words
    n = len(links) if n is None else n
    rec = np.asarray(records, dtype=np.uint64).reshape(-1)
    nrec = len(rec) // (W + 1) if nrec is None else nrec
    a = np.concatenate([np.asarray(prev_packed, dtype=np.uint64),
                        np.asarray([] if prev_gpos is None else prev_gpos, dtype=np.uint64)])
    b = np.concatenate([np.array([int(x) & M64 for x in links], dtype=np.uint64), rec])
    rc, s, res = _call(4, cfg, [n, nprev, nrec, rank, int(prev_gpos is not None), prev_counts, aft], a, b, [n * W],
                       [GUARD], 2 + NACT, aft)
    r = Result()
    if rc == 0:
        r.states = s[0].reshape(n, W)
        r.defer_err, r.next_cand, r.act_dist = int(res[0]), int(res[1]), [int(x) for x in res[2:]]
    return rc, r


def undo(cfg, packed, n, act_gen):
    """kind 5 -> (rc, act_gen after k_undo_gen)."""
    lib = kubecheck.load()
    par = np.array([n], dtype=np.uint64)
    a = np.ascontiguousarray(packed, dtype=np.uint64)
    b = np.array([int(x) & M64 for x in act_gen], dtype=np.uint64)
    res = np.full(len(b), GUARD, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))   # noqa: E731
    c = cfg.to_c()
    rc = lib.kc_shard_selftest(5, C.byref(c), p(par), 1, p(a), len(a), p(b), len(b), None, 0, None, 0, p(res),
                               len(res))
    return rc, [int(x) for x in res]


K_INSERT, K_INSERT_FIRST = 6, 7
PATH_TILES, PATH_SMALL, PATH_DEVICE = 0, 1, 2
RF_OUT, RF_CAND, RF_INSERTER, RF_DISPLACER = range(4)
DF_CAPACITY = 2
INS_SECTIONS = ("newmask", "rfp", "flag", "isnew", "wtot", "woff", "offsets", "ioff", "next", "link", "pkeys")
INS_GUARDS = (GUARD32, GUARD, GUARD32, GUARD32, GUARD32, GUARD32, GUARD32, GUARD32, GUARD, GUARD, GUARD)


def insert(kind, cfg, fr, records, *, level, nslots, world, rank, table=None, path=0, gpos=None, W=0, emit=1,
           cap=None, cap2=0, tail=1, unfused=0, next_gidx=0, aft=8, nrec=None):
    """kinds 6 / 7 -> (rc, Result).  fr: this rank's own parents (a Frontier or
    None); records: rows of state words + key.  On rc 0 the Result holds every
    section's live cells (guards verified), the final table and the counters."""
    SW = kubecheck.Spec(cfg).state_words
    n = fr.n if fr is not None else 0
    succ = fr.total() if fr is not None else 0
    rec = np.asarray(records, dtype=np.uint64).reshape(-1)
    nrec = len(rec) // (SW + 1) if nrec is None else nrec
    bound = succ + nrec
    tiles, rgrid = (n + TILE - 1) // TILE, (nrec + 255) // 256
    cells = (tiles if n else 0) + (rgrid if nrec else 0)
    tc = kind == K_INSERT_FIRST or path == PATH_TILES
    need = [n, nrec, nrec, nrec, cells + 8 if tc else 0, cells + 8 if tc else 0, 0 if tc else n, 0 if tc else nrec,
            0 if emit else bound * SW, bound if emit else 0, next_gidx + bound + 1]
    a = np.concatenate([fr.packed() if n else np.zeros(0, dtype=np.uint64),
                        np.asarray([] if gpos is None else gpos, dtype=np.uint64)])
    compact = kind == K_INSERT_FIRST and path == 1
    if table is None:
        table = np.zeros(nslots if compact else 2 * nslots, dtype=np.uint64)
    par = [n, nrec, level, nslots, world, rank, path, int(gpos is not None), emit, bound if cap is None else cap, tail,
           unfused, next_gidx, aft, cap2, W]
    rc, s, res = _call(kind, cfg, par, a, rec, need, INS_GUARDS, 8 + NACT + 10, aft, table=table)
    r = Result()
    r.table = table
    if rc == 0:
        for name, sec in zip(INS_SECTIONS, s):
            setattr(r, name, sec)
        r.next = r.next.reshape(-1, SW)
        names = ("err_key", "overflow", "probes", "chunk_base", "level_new", "cand_total", "defer_flags",
                 "first_defer_flags")
        for k, name in enumerate(names):
            setattr(r, name, int(res[k]))
        r.act_dist = [int(x) for x in res[8:8 + NACT]]
        r.head = [int(x) for x in res[8 + NACT:]]
        r.tiles, r.rgrid, r.bound = (tiles if n else 0), (rgrid if nrec else 0), bound
    return rc, r


def tlc(pkeys, links, other, W=None, aft=8, nn=None):
    """kind 2 -> (rc, Result: wmask, wbase, gnew, bits, brank, link, pkeys, gpos, overflow)."""
    W = len(other) if W is None else W
    nn = len(pkeys) if nn is None else nn
    a = np.array(list(pkeys) + list(links), dtype=np.uint64)
    rc, s, res = _call(2, None, [nn, W, aft], a, other, [W, W, nn, W + 1, W + 1, nn, nn, nn],
                       [GUARD32, GUARD32, GUARD32, GUARD32, GUARD32, GUARD, GUARD, GUARD32], 1, aft)
    r = Result()
    if rc == 0:
        r.wmask, r.wbase, r.gnew, r.bits, r.brank, r.link, r.pkeys, r.gpos = s
        r.overflow = int(res[0])
    return rc, r
