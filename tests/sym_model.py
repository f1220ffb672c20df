"""Host model of symmetry reduction, in the oracle's tuple space (numpy).

TEST INFRASTRUCTURE ONLY.  Independent of the product's packed form and of
its delta-swaps: a permutation acts on a canonical tuple (include/kubecheck.h:
word 0 = apiState as a mask over U, then 19 words per process) by
  * moving each actor's 19-word block to the actor's new index,
  * renaming the actors inside the version vector of every object value (the
    ovals at block offsets 2, 9 and 14: def | id<<1 | has_vv<<2 | spec<<3 | vv<<4),
  * moving every bit u of a U-mask (word 0 below bit 63, the lostUpdate ghost;
    each block's word 18, listRequests.objs) to the u whose vv is renamed,
    one bit at a time (u = id<<(A+1) | spec<<A | vv).
The orbit of a state is what the group makes of it; its canonical form is the
lexicographic minimum.  From the oracle's per-level state sets this gives what
a symmetric run must count (expected()).
"""
from __future__ import annotations

import itertools

import numpy as np

import pyoracle

PER_PROC = 19
OVALS = (2, 9, 14)
OBJS = 18
GHOST = np.uint64(1 << 63)
MASKS = {0: 0, "clients": 1, "controllers": 2, "actors": 3}


def group(nc: int, np_: int, mask: int):
    """Every permutation of the actors the mask allows, as tuples perm with
    perm[a] = the new index of actor a; the identity first."""
    cl = list(itertools.permutations(range(nc))) if (mask & 1) else [tuple(range(nc))]
    pv = list(itertools.permutations(range(nc, nc + np_))) if (mask & 2) else [tuple(range(nc, nc + np_))]
    return [c + p for c in cl for p in pv]


def _perm_vv(vv, perm):
    out = np.zeros_like(vv)
    for a, b in enumerate(perm):
        out |= ((vv >> np.uint64(a)) & np.uint64(1)) << np.uint64(b)
    return out


def _perm_mask(m, perm):
    A = len(perm)
    # (the ghost: never set in a block's objs word; no ghost when U has 64 bits)
    out = m & GHOST if A + 2 < 6 else np.zeros_like(m)
    for u in range(1 << (A + 2)):
        vv = u & ((1 << A) - 1)
        vv2 = sum(((vv >> a) & 1) << b for a, b in enumerate(perm))
        u2 = (u & ~((1 << A) - 1)) | vv2
        out |= ((m >> np.uint64(u)) & np.uint64(1)) << np.uint64(u2)
    return out


def permute(tuples, perm, nc: int, np_: int):
    t = np.atleast_2d(np.asarray(tuples, dtype=np.uint64))
    A = nc + np_
    assert len(perm) == A and sorted(perm) == list(range(A))
    assert all((a < nc) == (b < nc) for a, b in enumerate(perm)), "clients onto clients"
    out = t.copy()
    out[:, 0] = _perm_mask(t[:, 0], perm)
    for a, b in enumerate(perm):
        blk = t[:, 1 + PER_PROC * a: 1 + PER_PROC * (a + 1)].copy()
        for k in OVALS:
            ov = blk[:, k]
            blk[:, k] = (ov & np.uint64(15)) | (_perm_vv(ov >> np.uint64(4), perm) << np.uint64(4))
        blk[:, OBJS] = _perm_mask(blk[:, OBJS], perm)
        out[:, 1 + PER_PROC * b: 1 + PER_PROC * (b + 1)] = blk
    return out


def canon(tuples, nc: int, np_: int, mask: int):
    """The lexicographic minimum of every row's orbit."""
    t = np.atleast_2d(np.asarray(tuples, dtype=np.uint64))
    best = t.copy()
    rows = np.arange(len(t))
    for perm in group(nc, np_, mask)[1:]:
        p = permute(t, perm, nc, np_)
        diff = p != best
        first = diff.argmax(axis=1)
        less = diff.any(axis=1) & (p[rows, first] < best[rows, first])
        best[less] = p[less]
    return best


def _rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype((np.void, a.shape[1] * 8))).ravel()


def orbit_reps(tuples, nc: int, np_: int, mask: int):
    """One state (the first in the given order) of every orbit in `tuples`."""
    t = np.atleast_2d(np.asarray(tuples, dtype=np.uint64))
    if len(t) == 0:
        return t
    _, idx = np.unique(_rows(canon(t, nc, np_, mask)), return_index=True)
    return t[np.sort(idx)]


def canon_set(tuples, nc: int, np_: int, mask: int):
    """The canonical forms present in `tuples`, as a set of bytes."""
    t = np.atleast_2d(np.asarray(tuples, dtype=np.uint64))
    return set(r.tobytes() for r in canon(t, nc, np_, mask))


def orbit_widths(cfg, mask: int):
    """Orbits per BFS level of the oracle's run of cfg (to cfg.max_levels)."""
    return expected(cfg, mask, with_generated=False)["level_width"]


def expected(cfg, mask: int, with_generated: bool = True) -> dict:
    """What a run of cfg without an error must report under symmetry `mask`:
    level_width = orbits per level, distinct = their sum, depth unchanged,
    generated = the Init states (all of them, as without symmetry) + the
    successors of one state per orbit of every expanded level (every level,
    or levels 1 .. max_levels - 1 of a bounded run), act_gen = that sum per
    action.  Also states / states_width, the unreduced figures."""
    nc, np_ = cfg.nc, cfg.np
    ref = pyoracle.run(cfg)
    assert ref["err_kind"] == 0, "expected(): a run without an error"
    nlev = len(ref["level_width"])
    bounded = cfg.max_levels and nlev == cfg.max_levels and ref["queue_left"] > 0
    widths, gen = [], ref["init"]
    act = {a: 0 for a in pyoracle.ACTIONS}
    for lv in range(1, nlev + 1):
        t = pyoracle.level_tuples(cfg, lv)
        assert len(t) == ref["level_width"][lv - 1]
        reps = orbit_reps(t, nc, np_, mask)
        widths.append(len(reps))
        if with_generated and not (bounded and lv == nlev):
            for r in reps:
                succ, fail = pyoracle.successors(cfg, r)
                assert succ is not None, fail
                gen += len(succ)
                for a, _ in succ:
                    act[a] += 1
    out = {"level_width": widths, "distinct": sum(widths), "depth": ref["depth"], "init": ref["init"],
           "init_orbits": widths[0], "states": ref["distinct"], "states_width": ref["level_width"]}
    if with_generated:
        out["generated"] = gen
        out["act_gen"] = act
    return out
