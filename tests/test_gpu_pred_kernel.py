"""k_pred alone (csrc/pred_kernels.h) through kc_pred_selftest: made packed
states and hand-made or compiled programs; every answer is compared with the
host's evaluation of the same words (ctypes over pred.h's host path is
kc_pred_eval on tuples; here the words are made directly, so the expected
answers are computed in Python from the instruction semantics pred.h
documents), and the guard words around the result block must come back
intact."""
import ctypes as C

import numpy as np
import pytest

import kubecheck
from kubecheck import pred

pytestmark = pytest.mark.gpu

FORE, OUT_WORDS, AFT = 8, 10, 5
TILE = 1024                      # PRED_THREADS * PRED_PER_LANE
NONE = 2 ** 64 - 1
SIZES = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def fbits(word, shift, width):
    return (word << 8) | (shift << 16) | (width << 22)


def leaf_const(word, shift, width, cmp, c):
    return (pred.P_LEAF_CONST | (cmp << 4) | fbits(word, shift, width), c)


END = lambda k: (pred.P_END | (k << 8), 0)   # noqa: E731
EQ, NE, LT, LE, GT, GE = range(6)


def host_eval(code, w):
    """pred.h's documented semantics, restated: the mask of violated invariants of one state's words."""
    st, viol = [], 0
    cmpf = [lambda a, b: a == b, lambda a, b: a != b, lambda a, b: a < b, lambda a, b: a <= b,
            lambda a, b: a > b, lambda a, b: a >= b]

    def field(h):
        return (int(w[(h >> 8) & 0xff]) >> ((h >> 16) & 63)) & ((1 << ((h >> 22) & 127)) - 1)
    for h, x in code:
        op, c = h & 15, (h >> 4) & 7
        if op == pred.P_LEAF_CONST:
            st.append(cmpf[c](field(h), x))
        elif op == pred.P_LEAF_SET:
            a = field(h)
            st.append(a < 64 and bool((x >> a) & 1))
        elif op == pred.P_LEAF_FIELD:
            st.append(cmpf[c](field(h), field(h >> 24)))
        elif op == pred.P_LEAF_POPC:
            st.append(cmpf[c](bin(int(w[(h >> 8) & 0xff]) & x).count("1"), (h >> 32) & 0xff))
        elif op == pred.P_PUSH:
            st.append(bool(x & 1))
        elif op == pred.P_AND:
            b, a = st.pop(), st.pop()
            st.append(a and b)
        elif op == pred.P_OR:
            b, a = st.pop(), st.pop()
            st.append(a or b)
        elif op == pred.P_NOT:
            st.append(not st.pop())
        else:
            if not st.pop():
                viol |= 1 << ((h >> 8) & 7)
    assert not st
    return viol


def run_kernel(W, code, states, base=0):
    lib = kubecheck.load()
    words = np.array([x for ins in code for x in ins], dtype=np.uint64)
    states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, W)
    out = np.full(FORE + OUT_WORDS + AFT, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out[FORE:FORE + OUT_WORDS] = 0x1234            # junk the launch must reset, as a level's start does
    rc = lib.kc_pred_selftest(W, u64(words), len(code), u64(states), states.shape[0], base, u64(out), len(out))
    assert rc == 0, lib.kc_last_error()
    assert (out[:FORE] == 0xA5A5A5A5A5A5A5A5).all() and (out[FORE + OUT_WORDS:] == 0xA5A5A5A5A5A5A5A5).all()
    blk = [int(v) for v in out[FORE:FORE + OUT_WORDS]]
    return blk[0], blk[1], blk[2:]


def expect(code, states, base=0):
    key, counts = NONE, [0] * 8
    for i, w in enumerate(states):
        m = host_eval(code, w)
        for k in range(8):
            counts[k] += (m >> k) & 1
        if m:
            key = min(key, ((base + i) << 8) | ((m & -m).bit_length() - 1))
    return key, len(states), counts


def check(W, code, states, base=0):
    got = run_kernel(W, code, states, base)
    assert got == expect(code, states, base)
    return got


def made_states(W, n, seed=1):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2 ** 63, size=(n, W), dtype=np.uint64)
    s[:, 1] &= np.uint64(~0x1f & (2 ** 64 - 1))    # word 1's low five bits: 0 unless a test sets them
    return s


# word 1 bits 0..4 = 7 marks a violating state of invariant 0
MARK = [leaf_const(1, 0, 5, NE, 7), END(0)]


@pytest.mark.parametrize("W", [4, 6])
@pytest.mark.parametrize("n", SIZES)
def test_single_violator_positions(W, n):
    """One violating state at index 0, at the last index, and on both sides of every wave and tile boundary in range."""
    base_states = made_states(W, n, seed=n)
    spots = {0, n - 1} | {p for b in (64, TILE, 2 * TILE, 3 * TILE) for p in (b - 1, b) if p < n}
    for at in sorted(spots):
        s = base_states.copy()
        s[at, 1] |= np.uint64(7)
        key, ev, counts = check(W, MARK, s)
        assert key == (at << 8) and ev == n and counts[0] == 1


@pytest.mark.parametrize("W", [4, 6])
@pytest.mark.parametrize("n", SIZES)
def test_none_and_all_violating(W, n):
    s = made_states(W, n, seed=3)
    key, ev, counts = check(W, MARK, s)
    assert key == NONE and ev == n and counts == [0] * 8
    s[:, 1] |= np.uint64(7)
    key, ev, counts = check(W, MARK, s, base=5 * TILE)
    assert key == (5 * TILE) << 8 and ev == n and counts[0] == n


@pytest.mark.parametrize("W", [4, 6])
def test_two_invariants_min_key(W):
    """Two invariants violated by different states: the smaller index wins; on a state violating both, the smaller k."""
    code = [leaf_const(1, 0, 5, NE, 7), END(0), leaf_const(1, 0, 5, LT, 6), END(1)]     # 6 violates 1; 7 violates both
    n = 2 * TILE + 9
    s = made_states(W, n, seed=5)
    s[TILE + 3, 1] |= np.uint64(6)
    s[TILE + 70, 1] |= np.uint64(7)
    key, _, counts = check(W, code, s)
    assert key == ((TILE + 3) << 8 | 1) and counts[:2] == [1, 2]
    s[TILE + 3, 1] &= np.uint64(~6 & (2 ** 64 - 1))
    key, _, counts = check(W, code, s)
    assert key == ((TILE + 70) << 8 | 0) and counts[:2] == [1, 1]


@pytest.mark.parametrize("W", [4, 6])
def test_leaf_kinds(W):
    n = 300
    s = made_states(W, n, seed=7)
    last = W - 1
    # a field in the upper half of the last word (an objs mask lives there)
    s[:, last] &= np.uint64(0xFFFFFFFF)
    s[17, last] |= np.uint64(0x8001) << np.uint64(48)
    code = [leaf_const(last, 48, 16, EQ, 0), END(0)]
    assert check(W, code, s)[0] == 17 << 8
    # a popcount leaf on word 0 with bit 63 set there: a mask without bit 63 must not count the ghost
    s[:, 0] = np.uint64(0b101)
    s[:, 0] |= np.uint64(1) << np.uint64(63)
    s[44, 0] |= np.uint64(0b10)
    code = [(pred.P_LEAF_POPC | (LE << 4) | (0 << 8) | (2 << 32), 0xFFFF), END(0)]
    key, _, counts = check(W, code, s)
    assert key == 44 << 8 and counts[0] == 1
    # a two-field leaf: word 2 bits 8..11 against word 3 bits 20..23
    s[:, 2] = np.uint64(0x500)
    s[:, 3] = np.uint64(0x500000)
    s[99, 3] = np.uint64(0x400000)
    code = [(pred.P_LEAF_FIELD | (EQ << 4) | fbits(2, 8, 4) | (fbits(3, 20, 4) << 24), 0), END(0)]
    assert check(W, code, s)[0] == 99 << 8
    code = [(pred.P_LEAF_FIELD | (GT << 4) | fbits(2, 8, 4) | (fbits(3, 20, 4) << 24), 0), pred_not(), END(0)]
    assert check(W, code, s)[0] == 99 << 8
    # a membership leaf with bit 63 of the set: a 6-bit field, value 63 is a member, 62 is not
    s[:, 2] = np.uint64(63)
    s[5, 2] = np.uint64(62)
    code = [(pred.P_LEAF_SET | fbits(2, 0, 6), 1 << 63), END(0)]
    assert check(W, code, s)[0] == 5 << 8
    # a 7-bit field holding 64 or more is a member of nothing
    s[:, 2] = np.uint64(1)
    s[6, 2] = np.uint64(65)
    code = [(pred.P_LEAF_SET | fbits(2, 0, 7), 0b10), END(0)]
    assert check(W, code, s)[0] == 6 << 8


def pred_not():
    return (pred.P_NOT, 0)


@pytest.mark.parametrize("W", [4, 6])
def test_longest_and_deepest_programs(W):
    n = TILE + 1
    s = made_states(W, n, seed=9)
    s[:, 1] |= np.uint64(3)
    s[n - 1, 1] ^= np.uint64(1)
    # 128 instructions: 8 invariants of 15 leaves and connectives each, then END
    code = []
    for k in range(8):
        code.append(leaf_const(1, 0, 2, EQ, 3))
        for _ in range(7):
            code += [leaf_const(1, 1, 1, EQ, 1), (pred.P_AND, 0)]
        code.append(END(k))
    assert len(code) == pred.MAX_INSTR
    key, _, counts = check(W, code, s)
    assert key == (n - 1) << 8 and counts == [1] * 8
    # nesting depth 32: 32 leaves pushed, then 31 ANDs
    code = [leaf_const(1, 0, 2, EQ, 3)] * 32 + [(pred.P_AND, 0)] * 31 + [END(0)]
    key, _, counts = check(W, code, s)
    assert key == (n - 1) << 8 and counts[0] == 1


def test_against_kc_pred_eval_on_model_states():
    """Compiled programs on Model_1's first levels: the kernel, kc_pred_eval and pred.evaluate agree state by state."""
    import pyoracle
    import pred_model
    lib = kubecheck.load()
    sp = kubecheck.Spec(kubecheck.ModelConfig())
    cfg = pyoracle.config()
    tuples = np.concatenate([pyoracle.level_tuples(cfg, L) for L in range(1, 12)])
    packed = np.stack([sp.pack(t) for t in tuples])
    names = ["StoreAtMostOne", "NeverC4", "NotBothPending", "Mixed", "ReadBy", "OpsAgree"]
    prog = pred.compile_invariants({k: pred_model.EXAMPLES_M1[k] for k in names})
    code = prog.code
    key, ev, counts = check(sp.state_words, code, packed)
    words = (C.c_uint64 * len(prog.words))(*prog.words)
    host = [lib.kc_pred_eval(C.byref(sp._c), words, prog.n_instr, u64(np.ascontiguousarray(t))) for t in tuples]
    assert min(host) >= 0
    asts = [pred.parse(pred_model.EXAMPLES_M1[k]) for k in names]
    model = [sum((not pred.evaluate(a, t)) << k for k, a in enumerate(asts)) for t in tuples]
    assert host == model
    assert counts[:len(names)] == [sum((m >> k) & 1 for m in host) for k in range(len(names))]
    assert ev == len(tuples) and key != NONE


@pytest.mark.parametrize("model,W,exprs", [
    ((1, 2, 1), 6, ['Cardinality(apiState) = 0', r'\A p \in Controllers : pc[p] # "PVCListedPVCs"',
                    'Cardinality(listRequests["PVCController2"].objs) # 1']),
    ((2, 2, 1), 10, ['Cardinality(apiState) = 0', r'\A c \in Clients : pc[c] # "C1" \/ shouldReconcile[c]',
                     'Cardinality(listRequests["PVCController2"].objs) # 1',
                     r'Cardinality({o \in apiState : o.k = "PVC" /\ "PVCController2" \in o.vv}) = 0']),
])
def test_wider_states_against_kc_pred_eval_on_the_same_words(model, W, exprs):
    """W = 6 and W = 10 (four actors: 64 objects fill word 0, an objs mask per word): kc_pred_eval on the tuple
    of each packed state gives the kernel's key and counters."""
    import pyoracle
    lib = kubecheck.load()
    sp = kubecheck.Spec(kubecheck.ModelConfig(nc=model[0], np=model[1], ns=model[2]))
    assert sp.state_words == W
    cfg = pyoracle.config(*model)
    tuples = np.concatenate([pyoracle.level_tuples(cfg, L) for L in range(1, 9)])
    # hand-made: bit 63 of word 0 (the ghost at W = 6, the object u = 63 at W = 10) on a copy of the last states
    edge = tuples[-70:].copy()
    edge[:, 0] |= np.uint64(1 << 63)
    tuples = np.concatenate([tuples, edge])
    packed = np.stack([sp.pack(t) for t in tuples])
    prog = pred.compile_invariants(exprs, *model)
    key, ev, counts = check(W, prog.code, packed, base=3)
    words = (C.c_uint64 * len(prog.words))(*prog.words)
    host = [lib.kc_pred_eval(C.byref(sp._c), words, prog.n_instr, u64(np.ascontiguousarray(t))) for t in tuples]
    assert min(host) >= 0 and ev == len(tuples)
    assert counts[:len(exprs)] == [sum((m >> k) & 1 for m in host) for k in range(len(exprs))]
    first = next(i for i, m in enumerate(host) if m)
    assert key == ((3 + first) << 8) | ((host[first] & -host[first]).bit_length() - 1)
    asts = [pred.parse(e, *model) for e in exprs]
    assert host == [sum((not pred.evaluate(a, t, *model)) << k for k, a in enumerate(asts)) for t in tuples]
