"""The table-driven label lowering (kubeapi_spec.h: label_action, the packed
per-label successor counts of slot_count, the select-only plan) against the
CPU oracle, state by state, on the host build of the same header.

Every state of each walk is expanded by kc_spec_successors and by the
oracle's ko_successors into buffers pre-filled with a sentinel, so that for a
state whose enabled action raises an Assert the two also agree on the Assert
position: how many successors were listed before it, which they were, and
the failing action.  Compared per state: the number of successors, their
order, each one's action id and canonical tuple.  kc_spec_check and
kc_spec_fingerprint run on every state met: the first violated invariant and
its level must be the fixture's, fingerprints of distinct states must differ,
and the kernels' incremental fingerprint must equal the full one."""
import ctypes as C

import numpy as np
import pytest

from kubecheck import ModelConfig, Spec
from kubecheck._lib import ACTIONS

CAP = 64
SENTINEL = -7


class Walk:
    def __init__(self, oracle, nc, np_, ns, **flags):
        self.sp = Spec(ModelConfig(nc=nc, np=np_, ns=ns, **flags))
        self.ocfg = oracle.config(nc, np_, ns, **flags)
        self.klib, self.olib = self.sp._lib, oracle.lib()
        self.w = self.sp.tuple_words
        assert self.w == self.olib.ko_tuple_words(C.byref(self.ocfg))
        self.init = self.sp.init()
        assert (self.init == oracle.level_tuples(self.ocfg, 1)).all()
        u64p = C.POINTER(C.c_uint64)
        self.pa, self.oa = (C.c_int * CAP)(), (C.c_int * CAP)()
        self.pacts, self.oacts = np.frombuffer(self.pa, dtype=np.int32), np.frombuffer(self.oa, dtype=np.int32)
        self.pout, self.oout = np.zeros((CAP, self.w), np.uint64), np.zeros((CAP, self.w), np.uint64)
        self.pp, self.op = self.pout.ctypes.data_as(u64p), self.oout.ctypes.data_as(u64p)
        self.u64p = u64p
        self.act_gen = np.zeros(len(ACTIONS), np.int64)
        self.asserts = []         # (level, action, position) of every Assert met
        self.violation = None     # (level, invariant index) of the first invariant violated
        self.fps = set()          # fingerprints of the states met

    def expand(self, s, level):
        """The successors of s by both, compared; None if an Assert stopped the list."""
        sp_ = s.ctypes.data_as(self.u64p)
        self.pacts[:] = SENTINEL
        self.oacts[:] = SENTINEL
        pf, of = C.c_int(-1), C.c_int(-1)
        pn = self.klib.kc_spec_successors(C.byref(self.sp._c), sp_, self.pa, self.pp, CAP, C.byref(pf))
        on = self.olib.ko_successors(C.byref(self.ocfg), sp_, self.oa, self.op, CAP, C.byref(of))
        assert pf.value == of.value, ("failing action", pf.value, of.value)
        assert (pn == -2) == (on < 0) and (pn == -2 or pn == on), ("successor count", pn, on)
        assert np.array_equal(self.pacts, self.oacts), "action ids (or the Assert position)"
        n = int((self.pacts != SENTINEL).sum())
        assert (self.pacts[:n] != SENTINEL).all()
        assert np.array_equal(self.pout[:n], self.oout[:n]), "successor tuples"
        assert self.klib.kc_spec_fp_selfcheck(C.byref(self.sp._c), sp_) == 0
        np.add.at(self.act_gen, self.pacts[:n], 1)
        if pn == -2:
            self.asserts.append((level, ACTIONS[pf.value], n))
            return None
        assert n == pn
        return self.pout[:n]

    def meet(self, x, level):
        """kc_spec_check and kc_spec_fingerprint of a state first seen at `level`."""
        xp = x.ctypes.data_as(self.u64p)
        r = self.klib.kc_spec_check(C.byref(self.sp._c), xp)
        assert r >= -1
        if r >= 0 and (self.violation is None or level < self.violation[0]):
            self.violation = (level, r)
        fp = C.c_uint64()
        assert self.klib.kc_spec_fingerprint(C.byref(self.sp._c), xp, C.byref(fp)) == 0
        assert 0 < fp.value < 2**63
        self.fps.add(fp.value)

    def run(self, max_levels=0, max_states=0):
        """BFS from Init; returns the level widths.  States past an invariant
        violation are still expanded (the walk is about the lowering)."""
        seen, frontier = set(), []
        for x in self.init:
            seen.add(x.tobytes())
            self.meet(x, 1)
            frontier.append(x.copy())
        widths, level, expanded = [], 1, 0
        while frontier and (not max_levels or level <= max_levels) and (not max_states or expanded < max_states):
            widths.append(len(frontier))
            nxt = []
            for s in frontier:
                succ = self.expand(s, level)
                expanded += 1
                if succ is None:
                    continue
                for x in succ:
                    k = x.tobytes()
                    if k not in seen:
                        seen.add(k)
                        self.meet(x, level + 1)
                        nxt.append(x.copy())
            frontier, level = nxt, level + 1
        self.expanded = expanded
        self.distinct = len(seen)
        return widths


def _fingerprints_distinct(wk):
    # (a collision of two states shows as fewer fingerprints than states)
    assert len(wk.fps) == wk.distinct, ("fingerprint collisions", wk.distinct - len(wk.fps))


@pytest.mark.parametrize("can_fail,can_timeout", [(True, True), (False, True), (True, False), (False, False)])
def test_model1_every_state(oracle, fixtures, can_fail, can_timeout):
    key = "model1" if can_fail and can_timeout else f"model1_fail{int(can_fail)}_timeout{int(can_timeout)}"
    fx = fixtures[key]
    wk = Walk(oracle, 1, 1, 1, can_fail=can_fail, can_timeout=can_timeout)
    widths = wk.run()
    assert widths == fx["level_width"] and wk.expanded == fx["distinct"] == wk.distinct
    assert not wk.asserts and wk.violation is None
    assert {a: int(wk.act_gen[i]) for i, a in enumerate(ACTIONS)} == fx["act_gen"]
    _fingerprints_distinct(wk)
    if can_fail and can_timeout:
        assert wk.expanded == 163408
        # every label of both process kinds was exercised
        assert all(wk.act_gen[i] > 0 for i in range(len(ACTIONS))), "an action never occurred"
        assert len(ACTIONS) == 22


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_seeded_variants(oracle, fixtures, variant):
    """Every state the checker reaches under a seeded bug: up to the level of
    its error (variant 1 has none under TypeOK and OnlyOneVersion)."""
    fx = fixtures[f"variant{variant}"]
    depth = len(fx["level_width"])
    wk = Walk(oracle, 1, 1, 1, variant=variant)
    widths = wk.run(max_levels=max(depth, 1))
    assert widths[:depth] == fx["level_width"]
    _fingerprints_distinct(wk)
    if fx["err_kind"] == 0:
        assert widths == fx["level_width"] and wk.expanded == fx["distinct"]
        assert not wk.asserts and wk.violation is None
        assert {a: int(wk.act_gen[i]) for i, a in enumerate(ACTIONS)} == fx["act_gen"]
    elif fx["err_kind"] == 1:                                  # an Assert: its level, action and position
        assert wk.violation is None
        assert wk.asserts and min(a[0] for a in wk.asserts) == fx["err_level"]
        assert {a[1] for a in wk.asserts} == {fx["err_action"]}
    else:                                                      # an invariant: its level and index
        assert not wk.asserts
        assert wk.violation == (fx["err_level"], fx["err_invariant"])


def test_two_clients(oracle, fixtures):
    """Two actors of one kind (the per-actor action map by selects), up to the
    C4 Assert at level 10."""
    fx = fixtures["nc2"]
    wk = Walk(oracle, 2, 1, 1)
    widths = wk.run(max_levels=10)
    assert widths == fx["level_width"] and wk.expanded == sum(fx["level_width"])
    assert wk.violation is None
    assert wk.asserts and {(a[0], a[1]) for a in wk.asserts} == {(10, "C4")}
    _fingerprints_distinct(wk)


def test_two_controllers_first_levels(oracle, fixtures):
    """NP=2 (the benchmark's model): its first 31 levels, 195,563 states."""
    fx = fixtures["np2_40levels"]
    levels = 31
    assert sum(fx["level_width"][:levels]) == 195563
    wk = Walk(oracle, 1, 2, 1)
    widths = wk.run(max_levels=levels)
    assert widths == fx["level_width"][:levels]
    assert not wk.asserts and wk.violation is None
    _fingerprints_distinct(wk)
