"""Host model of k_claim and the settle passes (csrc/engine_kernels.h), and
the binding of kc_claim_selftest (csrc/claim_selftest.hip).  Helper module, no
tests here.

Nothing of the kernel's structure is in the model: no LDS table, no dealing,
no candidate lists.  A frontier is a list of parents; parent i has successors
(action, state) at positions t = 0, 1, ... in TLC order; a copy (i, t) carries
the fingerprint of its state and the claim key rank << 40 | (base + i) << 8 | t.
Tiles appear only where the kernel's outputs are per tile (256 parents).

  exact       the seen-set keeps, per fingerprint, the minimum claim (level <<
              44 | key) over what was pre-loaded and every copy; the copy that
              holds it is new iff the fingerprint was absent or held a larger
              claim of the same level.  Schedule-independent.
  first-claim some one copy of every absent fingerprint is new (the device's
              choice), none of a present one.
  sharded     as exact, over the fingerprints `rank` owns (kc_shard_owner of
              the owner-projected fingerprint); of every other fingerprint the
              smallest copy in each tile is that tile's representative: marked
              in repmask, counted per owner, staged as a record.
  counters    act_gen = successors per action; err_key = the minimum of
              (base + i) << 16 | position << 8 | 1 over Assert parents (position =
              the successors before the failing action) and (base + i) << 16 | 3
              over parents without successors when deadlocks are checked;
              probes = per tile, its distinct (owned) fingerprints.
  deferred    parent i is successor `position` of state `parent` of the previous
              frontier (link[i] = parent << 8 | position).

Successors, actions, fingerprints and invariants come from kubecheck.Spec, the
owner from kc_shard_owner, slot arithmetic (pre-loaded table images only) from
probe_model."""
import ctypes as C
import functools

import numpy as np

import kubecheck
import probe_model as pm
from kubecheck._lib import ACTIONS

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
TILE = 256
RCAP = 256                    # CLAIM_RCAP
CSUM_TILES = 64
LDS, LDS_SH = 2048, 1792      # CLAIM_LDS, CLAIM_LDS_SH
RANK_SHIFT = 40               # CLAIM_RANK_SHIFT
KEY_BITS = 44
E_ASSERT, E_INVARIANT, E_DEADLOCK = 1, 2, 3
DF_INVARIANT, DF_STAGE = 1, 4
FORE = 8
NACT = len(ACTIONS)
K_EXACT, K_FIRST, K_FIRST_C8, K_SHARD = range(4)
PF_DEFER, PF_PREV_COUNTS, PF_CSUM = 1, 2, 4
GUARD, GUARD32, GUARD8 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5
SECTIONS = ("newmask", "rcount", "ttot", "csum", "dfout", "counts_out", "repmask", "cnt", "tcnt", "stoff", "stage",
            "records")
SEC_GUARD = dict(newmask=GUARD32, rcount=GUARD32, ttot=GUARD32, csum=GUARD32, dfout=GUARD, counts_out=GUARD,
                 repmask=GUARD32, cnt=GUARD8, tcnt=GUARD32, stoff=GUARD, stage=GUARD, records=GUARD)
_ACT = {a: k for k, a in enumerate(ACTIONS)}


def popcount(x):
    return bin(int(x)).count("1")


@functools.lru_cache(maxsize=None)
def owner(fp, world):
    return kubecheck.load().kc_shard_owner(fp, world)


def make_claim(level, key):
    return (level << KEY_BITS) | key


class Parent:
    """One distinct parent: its successors as (action index, tuple, fingerprint,
    owner-projected fingerprint), the position of an Assert failure (or None),
    its packed words."""

    def __init__(self, spec, tup):
        self.tuple = np.ascontiguousarray(tup, dtype=np.uint64)
        self.packed = spec.pack(self.tuple)
        succ, fail = spec.successors(self.tuple)
        self.fail_pos = None
        if fail is not None:
            # kc_spec_successors stores the successors before the failing
            # action and returns -2: count the rows it wrote
            cap = 64
            acts = (C.c_int * cap)()
            out = np.full((cap, spec.tuple_words), M64, dtype=np.uint64)
            f = C.c_int(-1)
            rc = spec._lib.kc_spec_successors(C.byref(spec._c), self.tuple.ctypes.data_as(C.POINTER(C.c_uint64)), acts,
                                              out.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(f))
            assert rc == -2
            k = int((out != np.uint64(M64)).any(axis=1).sum())
            assert (out[:k] != np.uint64(M64)).any(axis=1).all()
            succ = [(ACTIONS[acts[j]], out[j].copy()) for j in range(k)]
            self.fail_pos = k
        self.succ = [(_ACT[a], x.copy(), spec.fingerprint(x), spec.fingerprint_own(x)) for a, x in succ]
        assert len(self.succ) <= 32


class Frontier:
    """n parents: a block of distinct tuples and, per parent, its block index
    (a frontier may repeat parents; the kernel sees only states)."""

    def __init__(self, spec, tuples, index=None):
        self.spec = spec
        tuples = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, spec.tuple_words)
        self.block = [Parent(spec, t) for t in tuples]
        self.index = list(range(len(self.block))) if index is None else [int(k) for k in index]
        self.n = len(self.index)
        self.tiles = (self.n + TILE - 1) // TILE

    def parent(self, i):
        return self.block[self.index[i]]

    def packed(self):
        return np.concatenate([self.parent(i).packed for i in range(self.n)])

    def copies(self, own=False):
        """(i, t, fingerprint, action) of every copy, in (parent, position) order."""
        for i in range(self.n):
            for t, (a, _, fp, fpo) in enumerate(self.parent(i).succ):
                yield i, t, (fpo if own else fp), a

    def total(self):
        return sum(len(self.parent(i).succ) for i in range(self.n))

    def fps(self, own=False):
        return {fp for _, _, fp, _ in self.copies(own)}

    def act_gen(self):
        g = [0] * NACT
        for _, _, _, a in self.copies():
            g[a] += 1
        return g

    def err_key(self, base, check_deadlock):
        k = M64
        for i in range(self.n):
            p = self.parent(i)
            if p.fail_pos is not None:
                k = min(k, (base + i) << 16 | p.fail_pos << 8 | E_ASSERT)
            elif not p.succ and check_deadlock:
                k = min(k, (base + i) << 16 | E_DEADLOCK)
        return k

    def tile_fps(self, own=False):
        """Per tile: {fingerprint: [(i, t, action), ...] in (parent, position) order}."""
        out = [dict() for _ in range(self.tiles)]
        for i, t, fp, a in self.copies(own):
            out[i // TILE].setdefault(fp, []).append((i, t, a))
        return out


def exact(fr, preload, level, base=0, rank=0, world=1):
    """-> (newmask[n], final {fingerprint: claim}, probes).  preload: {fp: claim}
    (any level up to `level`).  world > 1: only the fingerprints `rank` owns."""
    own = world > 1
    best = {}
    for i, t, fp, _ in fr.copies(own):
        if own and owner(fp, world) != rank:
            continue
        c = make_claim(level, rank << RANK_SHIFT | (base + i) << 8 | t)
        if fp not in best or c < best[fp][0]:
            best[fp] = (c, i, t)
    final = dict(preload)
    mask = [0] * fr.n
    for fp, (c, i, t) in best.items():
        old = preload.get(fp)
        if old is not None and (old >> KEY_BITS) < level:
            continue                       # an earlier level's: it keeps its claim
        if old is not None and old <= c:
            continue                       # a smaller claim of this level stays and wins
        final[fp] = c
        mask[i] |= 1 << t
    probes = sum(sum(1 for fp in d if not own or owner(fp, world) == rank) for d in fr.tile_fps(own))
    return mask, final, probes


def check_first(fr, present, mask, own=False):
    """The first-claim properties of a newmask array; present: the pre-loaded fingerprints."""
    assert len(mask) == fr.n
    winners = {}
    for i, t, fp, _ in fr.copies(own):
        if (int(mask[i]) >> t) & 1:
            winners[fp] = winners.get(fp, 0) + 1
    for i in range(fr.n):
        assert int(mask[i]) >> len(fr.parent(i).succ) == 0, ("a bit at or above the successor count", i)
    absent = fr.fps(own) - set(present)
    assert set(winners) == absent, (len(set(winners) - absent), "present fingerprints new;",
                                    len(absent - set(winners)), "absent ones not")
    twice = [fp for fp, k in winners.items() if k != 1]
    assert not twice, ("a fingerprint new more than once", len(twice))


def tile_popcounts(mask):
    return [sum(popcount(m) for m in mask[k:k + TILE]) for k in range(0, len(mask), TILE)]


def chunk_sums(ttot):
    return [sum(ttot[k:k + CSUM_TILES]) for k in range(0, len(ttot), CSUM_TILES)]


def representatives(fr, rank, world):
    """Per tile: the (i, t, action, owner) of the smallest copy of every
    fingerprint another rank owns, and all the remote copies."""
    reps, remote = [], []
    for d in fr.tile_fps(True):
        r, c = [], []
        for fp, cp in d.items():
            o = owner(fp, world)
            if o != rank:
                r.append(cp[0] + (o,))
                c += [x + (o,) for x in cp]
        reps.append(sorted(r))
        remote.append(sorted(c))
    return reps, remote


def masks_of(entries, n):
    m = [0] * n
    for e in entries:
        m[e[0]] |= 1 << e[1]
    return m


def staged_records(fr, repmask, rank, world):
    """The records of the marked copies per tile, in staging order: owner
    ascending, (parent, position) ascending within an owner; each (state
    words, key)."""
    out = []
    for tile in range(fr.tiles):
        recs = []
        for i in range(tile * TILE, min(fr.n, (tile + 1) * TILE)):
            for t, (a, x, _, fpo) in enumerate(fr.parent(i).succ):
                if (int(repmask[i]) >> t) & 1:
                    recs.append((owner(fpo, world), i, t, a, x))
        recs.sort(key=lambda r: r[:3])
        out.append([(o, list(fr.spec.pack(x)) + [rank << 60 | i << 16 | t << 8 | a]) for o, i, t, a, x in recs])
    return out


def deferred(prev, links):
    """The rebuild of a frontier from (parent, position) links into `prev` (a
    Frontier) -> dict(tuples, act_dist, defer_flags, defer_inv_n)."""
    spec = prev.spec
    r = dict(tuples=[], act_dist=[0] * NACT, defer_flags=0, defer_inv_n=0)
    first = None
    for i, (pp, t) in enumerate(links):
        a, x, _, _ = prev.parent(pp).succ[t]
        r["tuples"].append(x)
        r["act_dist"][a] += 1
        if first is None and spec.check_invariants(x) is not None:
            first = i
    if first is not None:
        r["defer_flags"] = DF_INVARIANT
        r["defer_inv_n"] = ~first & M64
    return r


def plan_sum(word):
    """The successor count a plan word holds: the sum of its 6-bit slot fields
    (bits 56 and up are not the plan's)."""
    w = int(word) & ((1 << 56) - 1)
    s = 0
    while w:
        s += w & 63
        w >>= 6
    return s


# ------------------------------------------------------------------ table images
def table_image(nslots, kind, entries):
    """The image of a table holding `entries` ({fp: ~claim word}, or fps for
    the compact table), each on its probe run."""
    t = pm.Table(nslots, "compact" if kind == K_FIRST_C8 else "wide")
    for fp in sorted(entries):
        i, found = t.locate(fp)
        assert i is not None and not found
        t.w[i * t.wps] = fp
        if t.wps == 2:
            t.w[2 * i + 1] = entries[fp]
    return np.array(t.w, dtype=np.uint64)


def table_entries(image, kind):
    """{fp: ~claim word} (compact: {fp: 0}) of an image; every fingerprint once."""
    w = np.asarray(image, dtype=np.uint64)
    if kind == K_FIRST_C8:
        fps, words = w, np.zeros(len(w), dtype=np.uint64)
    else:
        fps, words = w[0::2], w[1::2]
        assert not (words[fps == 0] != 0).any(), "a claim word in an empty slot"
    keep = fps != 0
    out = dict(zip((int(x) for x in fps[keep]), (int(x) for x in words[keep])))
    assert len(out) == int(keep.sum()), "a fingerprint stored twice"
    return out


def check_runs(image, kind):
    """Every stored fingerprint lies on its probe run before the first empty slot."""
    n = len(image) if kind == K_FIRST_C8 else len(image) // 2
    pm.Table(n, "compact" if kind == K_FIRST_C8 else "wide", image=image).check_runs()


# ----------------------------------------------------------------------- harness
class Result:
    pass


def selftest(kind, cfg, fr=None, *, packed=None, n=None, base=0, level=5, check_deadlock=1, spread=768, nslots=None,
             table=None, world=1, rank=0, flags=0, prev=None, links=None, stage_cap=0, aft=8):
    """One kc_claim_selftest call -> (rc, Result).  fr: the Frontier (or
    `packed` words and n); deferred: prev (a Frontier) and links [(parent,
    position)].  table: the image (zeros when None), changed in place.  On rc
    0 the Result holds every section's live cells (guards verified), the final
    table and the counters."""
    lib = kubecheck.load()
    W = kubecheck.Spec(cfg).state_words
    RW = None
    deferred_ = bool(flags & PF_DEFER)
    if deferred_:
        a = np.zeros(0, dtype=np.uint64)
        n = len(links) if n is None else n
        b = np.concatenate([prev.packed(), np.array([(pp << 8 | t) & M64 for pp, t in links], dtype=np.uint64)])
        nprev = prev.n
    else:
        a = fr.packed() if packed is None else np.ascontiguousarray(packed, dtype=np.uint64)
        n = (fr.n if fr is not None else len(a) // W) if n is None else n
        b = np.zeros(0, dtype=np.uint64)
        nprev = 0
    tiles = (n + TILE - 1) // TILE
    sh = kind == K_SHARD
    if sh:
        # Record<M>::RW: 64 key bits + the packed fields, in whole 16-B units (csrc/record.h)
        # (a wrong figure here makes the section sizes wrong: -EINVAL)
        RW = {1: 4, 2: 6, 3: 10}[cfg.np]
    need = [n, tiles, tiles, -(-tiles // CSUM_TILES) if flags & PF_CSUM else 0, (base + n) * W if deferred_ else 0,
            base + n if deferred_ else 0, n if sh else 0, world * n if sh else 0, world * tiles if sh else 0,
            tiles if sh else 0, stage_cap * RW if sh else 0, stage_cap * (W + 1) if sh else 0]
    at = [0]
    for k in need:
        at.append(at[-1] + FORE + k + aft)
    out = np.zeros(at[-1], dtype=np.uint64)
    for k, name in enumerate(SECTIONS):
        out[at[k]:at[k + 1]] = SEC_GUARD[name]
    out[at[3] + FORE:at[3] + FORE + need[3]] = 0           # csum is added into
    ntable = nslots if kind == K_FIRST_C8 else 2 * nslots
    if table is None:
        table = np.zeros(ntable, dtype=np.uint64)
    assert table.dtype == np.uint64 and table.flags.c_contiguous
    res = np.full(10 + 2 * NACT, GUARD, dtype=np.uint64)
    par = np.array([n, base, level, check_deadlock, spread, nslots, world, rank, flags, nprev, stage_cap, aft],
                   dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))   # noqa: E731
    c = cfg.to_c()
    rc = lib.kc_claim_selftest(kind, C.byref(c), p(par), len(par), p(a), len(a), p(b), len(b), p(table), len(table),
                               p(out), len(out), p(res), len(res))
    r = Result()
    r.table = table
    if rc != 0:
        return rc, r
    for k, name in enumerate(SECTIONS):
        sec = out[at[k]:at[k + 1]]
        g = np.uint64(SEC_GUARD[name])
        assert (sec[:FORE] == g).all(), (name, "fore guard")
        assert (sec[FORE + need[k]:] == g).all(), (name, "aft guard")
        setattr(r, name, sec[FORE:FORE + need[k]].copy())
    r.tiles, r.n, r.W, r.RW = tiles, n, W, RW
    names = ("err_key", "overflow", "probes", "settles", "cand_ovf", "next_cand", "defer_flags", "defer_inv_n",
             "ovf_count", "stage_cur")
    for k, name in enumerate(names):
        setattr(r, name, int(res[k]))
    r.act_gen = [int(x) for x in res[10:10 + NACT]]
    r.act_dist = [int(x) for x in res[10 + NACT:]]
    return rc, r
