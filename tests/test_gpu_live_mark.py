"""The two kernels of a user formula alone (csrc/live_prog.h k_live_mark_prog<W>,
csrc/live_graph.h k_live_first_trig) through kc_live_mark_selftest: made packed
states, made CSR graphs and levels, hand-made and compiled programs.  The
expected alive, terminal and trig bytes, the counters and the first state of
alive_in /\\ trig are a few lines of numpy over the same words; the guard
elements around every section must come back intact."""
import ctypes as C

import numpy as np
import pytest

import kubecheck
from kubecheck import pred

pytestmark = pytest.mark.gpu

FORE, AFT = 8, 5
GUARD, JUNK = 0xA5, 0x77
NONE = 0xffffffff
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
EQ = 0
MASK64 = 2 ** 64 - 1


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def fbits(word, shift, width):
    return (word << 8) | (shift << 16) | (width << 22)


def END(k):
    return (pred.P_END | (k << 8), 0)


# P: word 1 bits 0..4 = 7;  Q: the last word's bits 8..11 = 9 (the last word differs with W)
def marker_program(W):
    return [(pred.P_LEAF_CONST | (EQ << 4) | fbits(1, 0, 5), 7), END(0),
            (pred.P_LEAF_CONST | (EQ << 4) | fbits(W - 1, 8, 4), 9), END(1)]


def made_states(W, n, p_set, q_set, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2 ** 63, size=(n, W), dtype=np.uint64)
    s[:, 1] &= np.uint64(~0x1f & MASK64)
    s[:, W - 1] &= np.uint64(~0xf00 & MASK64)
    for i in p_set:
        s[i, 1] |= np.uint64(7)
    for i in q_set:
        s[i, W - 1] |= np.uint64(9 << 8)
    return s


def made_graph(n, seed):
    """Out-degrees 0..3; every fifth state has self-loops only, every seventh no edge at all."""
    rng = np.random.default_rng(seed + 1000)
    deg = rng.integers(0, 4, size=n)
    deg[::7] = 0
    edges = []
    for i in range(n):
        if i % 5 == 0:
            edges += [i] * int(deg[i])
        else:
            edges += [int(x) for x in rng.integers(0, n, size=int(deg[i]))]
    level = np.sort(rng.integers(1, 4, size=n))
    level[0] = 1
    return deg.astype(np.uint64), np.array(edges, dtype=np.uint64), level.astype(np.uint64)


def terminal_of(deg, edges):
    out, at = [], 0
    for i, d in enumerate(deg):
        out.append(all(int(e) == i for e in edges[at:at + int(d)]))
        at += int(d)
    return np.array(out, dtype=bool)


def run(W, form, code, states, deg, edges, level, alive_in):
    lib = kubecheck.load()
    n = states.shape[0]
    words = np.array([x for ins in code for x in ins], dtype=np.uint64)
    sec = FORE + n + AFT
    out = np.full(3 * sec, GUARD, dtype=np.uint64)
    for k in range(3):
        out[k * sec + FORE:k * sec + FORE + n] = JUNK
    res = np.full(5, 0x1234, dtype=np.uint64)
    par = np.array([W, form, n, AFT], dtype=np.uint64)
    edges_arg = edges if len(edges) else np.zeros(1, dtype=np.uint64)
    rc = lib.kc_live_mark_selftest(u64(par), 4, u64(words), len(code), u64(np.ascontiguousarray(states)), u64(deg),
                                   u64(edges_arg), len(edges), u64(level), u64(alive_in.astype(np.uint64)), u64(out),
                                   len(out), u64(res), 5)
    assert rc == 0, lib.kc_last_error()
    secs = []
    for k in range(3):
        blk = out[k * sec:(k + 1) * sec]
        assert (blk[:FORE] == GUARD).all() and (blk[FORE + n:] == GUARD).all(), f"section {k}: a guard was written"
        secs.append(blk[FORE:FORE + n])
    return secs, [int(x) for x in res]


def check(W, form, code, states, p_true, q_true, deg, edges, level, alive_in):
    """p_true / q_true: bool arrays, the program's predicates on every state as the host computes them."""
    (alive, terminal, trig), res = run(W, form, code, states, deg, edges, level, alive_in)
    stay = ~q_true
    want_trig = p_true if form == 0 else (level == 1)
    term = terminal_of(deg, edges)
    assert (alive == stay.astype(np.uint64)).all()
    assert (terminal == term.astype(np.uint64)).all()
    assert (trig == want_trig.astype(np.uint64)).all()
    both = alive_in.astype(bool) & want_trig
    first = int(np.flatnonzero(both)[0]) if both.any() else NONE
    assert res == [int(stay.sum()), int((stay & term).sum()), int((stay & want_trig).sum()), first, int(both.sum())]


def placements(n):
    """no state; every state; only index 0; only n - 1; only 63 and 64; only 255 and 256 (those in range)."""
    return [set(), set(range(n)), {0}, {n - 1}, {i for i in (63, 64) if i < n}, {i for i in (255, 256) if i < n}]


@pytest.mark.parametrize("W", [4, 6, 10])
@pytest.mark.parametrize("n", SIZES)
def test_mark_and_first_trigger(W, n):
    code = marker_program(W)
    deg, edges, level = made_graph(n, n)
    rng = np.random.default_rng(n * 31 + W)
    sets = placements(n)
    for k, p_set in enumerate(sets):
        q_set = sets[(k + 2) % len(sets)]
        states = made_states(W, n, p_set, q_set, seed=n + k)
        p_true = np.isin(np.arange(n), list(p_set))
        q_true = np.isin(np.arange(n), list(q_set))
        for form in (0, 1):
            # alive_in: random, nothing, and exactly the states of this placement
            for alive_in in (rng.integers(0, 2, size=n), np.zeros(n, dtype=np.int64), p_true.astype(np.int64)):
                check(W, form, code, states, p_true, q_true, deg, edges, level, alive_in)


@pytest.mark.parametrize("W", [4, 6, 10])
def test_first_is_the_smallest_index_across_waves_and_blocks(W):
    """alive_in /\\ trig on both sides of every wave and block boundary: the smallest index wins, every one is counted."""
    n = 1025
    code = marker_program(W)
    deg, edges, level = made_graph(n, 7)
    spots = [0, 63, 64, 255, 256, 257, 511, 512, 1023, 1024]
    for lo in range(len(spots)):
        p_set = set(spots[lo:])
        states = made_states(W, n, p_set, set(), seed=lo)
        p_true = np.isin(np.arange(n), list(p_set))
        alive_in = np.ones(n, dtype=np.int64)
        alive_in[spots[lo]] = lo % 2          # every other time the first trigger state is not alive: the next one wins
        check(W, 0, code, states, p_true, np.zeros(n, dtype=bool), deg, edges, level, alive_in)
    # form 1: the Init states are the trigger whatever P says
    level = np.full(n, 2, dtype=np.uint64)
    level[:3] = 1
    alive_in = np.ones(n, dtype=np.int64)
    alive_in[:2] = 0
    states = made_states(W, n, set(range(n)), {5}, seed=3)
    check(W, 1, code, states, np.ones(n, dtype=bool), np.isin(np.arange(n), [5]), deg, edges, level, alive_in)


@pytest.mark.parametrize("model,W,formula", [
    ((1, 1, 1), 4, r'"Client" \in DOMAIN requests ~> (pc["Client"] = "CStart" \/ Cardinality(apiState) >= 10)'),
    ((1, 2, 1), 6, r'(\E p \in Controllers : Cardinality(listRequests[p].objs) > 1) ~> requests["Client"].op = op["Client"]'),
    ((2, 2, 1), 10, r'<>(\A c \in Clients : pc[c] \in {"C1", "C5"} => shouldReconcile[c])'),
])
def test_compiled_programs_on_random_words(model, W, formula):
    """Every leaf kind the compiler emits, on random words: the expected bits are pred.h's documented semantics,
    restated in Python by tests/test_gpu_pred_kernel.py's host_eval."""
    from test_gpu_pred_kernel import host_eval
    form, prog = pred.compile_temporal(formula, *model)
    assert prog.W == W
    n = 300
    rng = np.random.default_rng(W)
    states = rng.integers(0, 2 ** 63, size=(n, W), dtype=np.uint64)
    states[: n // 2, 1:] &= np.uint64(0x0303030303030303)        # small field values: the comparisons go both ways
    bits = np.array([host_eval(prog.code, w) for w in states])
    p_true, q_true = (bits & 1) == 0, (bits & 2) == 0
    assert 0 < q_true.sum() < n
    deg, edges, level = made_graph(n, W)
    check(W, form, prog.code, states, p_true, q_true, deg, edges, level, rng.integers(0, 2, size=n))
