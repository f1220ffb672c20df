"""User-defined temporal formulas without a GPU: the shapes
pred.parse_temporal accepts and refuses, the compiled pair of predicates
(kc_pred_eval, the code k_live_mark_prog runs) against pred.evaluate on every
state of the three small graphs, the user spellings of the built-in properties
against live_model.stay, the expected-values table of tests/temporal_model.py,
and the argument checks of the new C entry points."""
import ctypes as C

import numpy as np
import pytest

import kubecheck
from kubecheck import ModelConfig, _lib, pred
from kubecheck.pred import PredError

import live_model
import temporal_model as tm

PC = 'pc["Client"]'


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def test_accepted_shapes():
    cstart, c2 = pred.parse(f'{PC} = "CStart"'), pred.parse(f'{PC} = "C2"')
    true = ("const", True)
    assert pred.parse_temporal(f'{PC} = "C2" ~> {PC} = "CStart"') == (0, c2, cstart)
    assert pred.parse_temporal(f'({PC} = "C2") ~> ({PC} = "CStart")') == (0, c2, cstart)
    assert pred.parse_temporal(f'(({PC} = "C2" ~> {PC} = "CStart"))') == (0, c2, cstart)
    assert pred.parse_temporal(f'[]({PC} = "C2" => <>{PC} = "CStart")') == (0, c2, cstart)
    assert pred.parse_temporal(f'[](({PC} = "C2") => <>({PC} = "CStart"))') == (0, c2, cstart)
    assert pred.parse_temporal(f'[]<>({PC} = "CStart")') == (0, true, cstart)
    assert pred.parse_temporal(f'[]<>{PC} = "CStart"') == (0, true, cstart)       # brackets next to []
    assert pred.parse_temporal(f'[] <> {PC} = "CStart"') == (0, true, cstart)
    assert pred.parse_temporal(f'<>({PC} = "CStart")') == (1, true, cstart)
    assert pred.parse_temporal(f'<>{PC} = "CStart" \\* a comment with ~> in it') == (1, true, cstart)
    # operands with =>, < and > comparisons, <=>, strings and sets: none of them is taken for ~> or <>
    lhs = f'({PC} = "C5" => Cardinality(apiState) >= 1)'
    rhs = '(Len(stack["Client"]) < 1 /\\ Cardinality(apiState) > 0)'
    assert pred.parse_temporal(f"{lhs} ~> {rhs}") == (0, pred.parse(lhs), pred.parse(rhs))
    lhs = f'({PC} = "C5" <=> Cardinality(apiState) =< 1)'
    rhs = f'{PC} \\in {{"CStart", "C1"}} \\/ Cardinality(apiState) <= 2'
    assert pred.parse_temporal(f"{lhs} ~> {rhs}") == (0, pred.parse(lhs), pred.parse(rhs))
    form, p_ast, q_ast = pred.parse_temporal(tm.SPELLINGS["SomeActorRestarts"], 1, 2, 1)
    assert form == 0 and p_ast == true
    assert q_ast == pred.parse(r'(\E c \in Clients : pc[c] = "CStart") \/ (\E p \in Controllers : pc[p] = "PVCStart")',
                               1, 2, 1)
    assert pred.parse_temporal(tm.REQUEST_RESTARTS)[1] == pred.parse(r'"Client" \in DOMAIN requests')
    assert pred.has_temporal(tm.C2_RESTARTS) and not pred.has_temporal(f'{PC} = "~> <> []"')


@pytest.mark.parametrize("text,words", [
    (f'<>[]({PC} = "C5")', ["<>[]", "SCC"]),
    (f'[]{PC} = "C1"', ["[]P", "INVARIANT"]),
    (f'[]({PC} = "C1")', ["[]P", "INVARIANT"]),
    (f'{PC} = "C1" ~> {PC} = "C2" ~> {PC} = "C3"', ["more than one temporal operator", "~>"]),
    (f'[]<>[]({PC} = "C1")', ["more than one temporal operator", "[]"]),
    (f'<>({PC} = "C1") ~> TRUE', ["more than one temporal operator"]),
    (f'{PC} = "C1" ~> (<>({PC} = "C2"))', ["<> inside an operand", "nested"]),
    (f'({PC} = "C1" ~> {PC} = "C2") /\\ TRUE', ["~> inside an operand"]),
    (f'TRUE /\\ <>({PC} = "C1")', ["<> combined with a connective"]),
    (f'[](({PC} = "C1") => <>[]({PC} = "C1"))', ["<>[]", "nested"]),
    (f'[]({PC} = "C1" /\\ <>({PC} = "C2"))', ["neither P => <>Q", "nested or combined"]),
    (f'[]{PC} = "C1" => <>({PC} = "C2")', ["unparenthesised", "combined"]),
    (f'[]<>{PC} = "C1" /\\ TRUE', ["parenthesise the operand of []<>"]),
    (f'{PC} = "C1" => TRUE ~> TRUE', ["parenthesise the operand of ~>"]),
    (f'{PC} = "C1"', ["no temporal operator", "a state predicate: list it under INVARIANT"]),
    ("", ["empty formula"]),
    (f'<>', ["<> lacks an operand"]),
    (f'{PC} = "C1" ~> ', ["~> lacks an operand"]),
    (f'<>({PC} = "C1"', ["unbalanced"]),
    (f'<>({PC} = "NoSuchLabel")', ["NoSuchLabel"]),                       # the operand's own error comes through
])
def test_refused_shapes_are_named(text, words):
    with pytest.raises(PredError) as e:
        pred.parse_temporal(text)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_compile_temporal_is_two_predicates():
    form, prog = pred.compile_temporal(tm.C2_RESTARTS)
    assert form == 0 and prog.names == ["trigger", "goal"]
    ends = [h for h, _ in prog.code if h & 15 == pred.P_END]
    assert [(h >> 8) & 0xff for h in ends] == [0, 1]
    form, prog = pred.compile_temporal(tm.EVENTUALLY_RECONCILED)
    assert form == 1 and prog.code[0] == (pred.P_PUSH, 1)                # P = TRUE
    with pytest.raises(PredError):
        pred.compile_temporal('pc["Client"] = "C2"')


FORMULAS = {name: sorted({f for n, f, *_ in tm.ROWS if n == name}) for name in live_model.MODELS}


@pytest.mark.parametrize("name", list(live_model.MODELS))
def test_program_bits_equal_evaluate_on_every_state(oracle, name):
    """kc_pred_eval's two bits (bit k = predicate k is FALSE) are pred.evaluate(P) and pred.evaluate(Q) negated."""
    lib = kubecheck.load()
    m = live_model.model(oracle, name)
    mod = tm.procs_of_model(name)
    cfg = ModelConfig(**live_model.MODELS[name]).to_c()
    tuples = np.array(m.states, dtype=np.uint64)
    formulas = FORMULAS[name] + [tm.SPELLINGS[k] for k in ("ReconcileCompletes", "ClientRestarts")]
    assert len(formulas) >= 4
    for f in formulas:
        form, p_ast, q_ast = pred.parse_temporal(f, *mod)
        form2, prog = pred.compile_temporal(f, *mod)
        assert form2 == form
        words = prog.array()
        for i in range(len(tuples)):
            got = lib.kc_pred_eval(C.byref(cfg), u64(words), prog.n_instr, u64(tuples[i]))
            want = (not pred.evaluate(p_ast, m.states[i], *mod)) | (not pred.evaluate(q_ast, m.states[i], *mod)) << 1
            assert got == want, (f, i)


@pytest.mark.parametrize("name", list(live_model.MODELS))
def test_user_spellings_give_the_builtin_stay_sets(oracle, name):
    m = live_model.model(oracle, name)
    mod = tm.procs_of_model(name)
    for pname, formula in tm.SPELLINGS.items():
        if pname == "SomeActorRestarts" and mod[1] == 0:
            formula = tm.SPELLING_NO_CONTROLLERS
        form, p_ast, q_ast = pred.parse_temporal(formula, *mod)
        prop = live_model.PROPERTIES.index(pname)
        assert form == 0
        for t in m.states:
            assert (not pred.evaluate(q_ast, t, *mod)) == live_model.stay(prop, t, mod[0], mod[1]), (pname, t)
            # ReconcileCompletes' trigger is its own stay set; the other two trigger everywhere
            assert pred.evaluate(p_ast, t, *mod) == (live_model.stay(prop, t, mod[0], mod[1]) if prop == 0 else True)


@pytest.mark.parametrize("row", tm.ROWS, ids=[f"{r[0]}-{k}" for k, r in enumerate(tm.ROWS)])
def test_table_literals_are_what_the_model_computes(oracle, row):
    name, formula, n_stay, n_trig_stay, nxt, proc = row
    m = live_model.model(oracle, name)
    v = tm.check(m, name, formula, "next")
    first = v.first
    assert (len(v.stay), len(v.stay & v.trigger)) == (n_stay, n_trig_stay)
    assert (len(v.live), len(v.live_trigger), None if first is None else m.level[first], first, v.rounds) == nxt
    v = tm.check(m, name, formula, "process")
    first = v.first
    assert (len(v.fair.fair), len(v.live), len(v.live_trigger), None if first is None else m.level[first], first) == proc


def test_the_table_has_a_trigger_that_matters(oracle):
    """L is not empty and yet the property holds; the first state of L /\\ T is not L's first."""
    m = live_model.model(oracle, "nofaults_111")
    v = tm.check(m, "nofaults_111", tm.C5_RECONCILED, "next")
    assert v.live and not v.violated
    v = tm.check(m, "nofaults_111", tm.C2_RESTARTS, "next")
    assert min(m.level[i] for i in v.live) == 2 and m.level[v.first] == 24
    m = live_model.model(oracle, "default_101")
    v = tm.check(m, "default_101", tm.EVENTUALLY_RECONCILED, "next")
    assert v.first == 1 and 0 in v.trigger and 0 not in v.live


def test_python_front_end_without_a_gpu():
    with pytest.raises(ValueError, match="not both"):
        kubecheck.LivenessChecker(ModelConfig(), "ClientRestarts", formula=tm.C2_RESTARTS)
    with pytest.raises(PredError, match="INVARIANT"):                  # compiled before anything is created
        kubecheck.LivenessChecker(ModelConfig(), formula='pc["Client"] = "C2"')
    with pytest.raises(PredError, match="<>\\[\\]"):
        kubecheck.LivenessChecker(ModelConfig(), formula='<>[](pc["Client"] = "C2")')
    r = kubecheck.LiveResult(
        property="ReconcileCompletes", states=3, edges=3, init=1, depth=3, stay_states=2, live_states=2,
        live_terminal=0, rounds=1, error=None, error_action=None, error_self=-1, violated=True,
        kind="back-to-state", prefix_len=2, trace_len=3, loop_start=1, seconds=0.0, build_ms=0.0, trim_ms=0.0)
    assert (r.formula, r.trigger_stay, r.trigger_live) == (None, 0, 0)
    assert (_lib.LIVE_USER, _lib.LIVE_FORMS) == (-1, ("leads-to", "eventually"))


def mark_args(W=4, form=0, n=3, aft=2, code=None, deg=(1, 0, 2), edges=(1, 0, 2), level=(1, 2, 2), alive=(1, 0, 1)):
    code = code if code is not None else [(pred.P_PUSH, 1), (pred.P_END, 0), (pred.P_PUSH, 0), (pred.P_END | (1 << 8), 0)]
    words = np.array([x for ins in code for x in ins], dtype=np.uint64)
    arr = lambda v: np.array(v, dtype=np.uint64)       # noqa: E731
    out = np.zeros(3 * (8 + n + aft), dtype=np.uint64)
    res = np.zeros(5, dtype=np.uint64)
    return dict(par=arr([W, form, n, aft]), words=words, n_instr=len(code), states=np.zeros(max(n, 1) * W, dtype=np.uint64),
                deg=arr(deg), edges=arr(edges), level=arr(level), alive=arr(alive), out=out, res=res)


def call_mark(a, **over):
    lib = kubecheck.load()
    a = dict(a, **over)
    return lib.kc_live_mark_selftest(u64(a["par"]), len(a["par"]), u64(a["words"]), a["n_instr"], u64(a["states"]),
                                     u64(a["deg"]), u64(a["edges"]), len(a["edges"]), u64(a["level"]), u64(a["alive"]),
                                     u64(a["out"]), len(a["out"]), u64(a["res"]), len(a["res"]))


def test_c_side_argument_checks_need_no_gpu():
    lib = kubecheck.load()
    words = (C.c_uint64 * 8)()
    assert lib.kc_live_set_formula(None, 0, words, 4) == -22
    assert b"kc_live_set_formula" in lib.kc_last_error()
    assert lib.kc_live_trigger_counts(None, None, None) == -22
    # kc_live_create_formula checks the formula before it touches the device
    c = ModelConfig().to_c()
    h = C.c_void_p()
    form, prog = pred.compile_temporal(tm.C2_RESTARTS)
    one = pred.compile_invariants(["TRUE"])
    three = pred.compile_invariants(["TRUE", "TRUE", "FALSE"])
    user, builtin = _lib.KcLiveConfig(_lib.LIVE_USER, 0), _lib.KcLiveConfig(2, 0)
    for live, f, p, why in ((user, 0, one, b"exactly two"), (user, 0, three, b"exactly two"), (user, 2, prog, b"form"),
                            (builtin, 0, prog, b"not KC_LIVE_USER"),
                            (_lib.KcLiveConfig(_lib.LIVE_USER, 0, 7), 0, prog, b"fairness")):
        assert lib.kc_live_create_formula(C.byref(c), C.byref(live), f, u64(p.array()), p.n_instr, C.byref(h)) == -22
        assert why in lib.kc_last_error() and not h.value, why
    assert lib.kc_live_create_formula(C.byref(c), C.byref(user), 0, None, 4, C.byref(h)) == -22
    assert lib.kc_live_create(C.byref(c), C.byref(user), C.byref(h)) == -22          # no formula, no handle
    assert b"kc_live_create_formula" in lib.kc_last_error()
    # a program for another model's state width: its word indices are checked against this model's W
    wide = pred.compile_temporal(r'<>(Cardinality(listRequests["PVCController2"].objs) = 1)', 2, 2, 1)[1]
    assert lib.kc_live_create_formula(C.byref(c), C.byref(user), 1, u64(wide.array()), wide.n_instr, C.byref(h)) == -22
    assert b"field outside the state" in lib.kc_last_error() or b"word index" in lib.kc_last_error()
    assert lib.kc_live_mark_selftest(None, 0, None, 0, None, None, None, 0, None, None, None, 0, None, 0) == -22
    good = mark_args()
    assert call_mark(good) in (0, -19)                                  # good input: only the GPU can be missing
    end0, end1 = (pred.P_END, 0), (pred.P_END | (1 << 8), 0)
    push = (pred.P_PUSH, 1)
    bad = [
        (dict(par=np.array([5, 0, 3, 2], dtype=np.uint64)), b"W is 4, 6 or 10"),
        (dict(par=np.array([4, 2, 3, 2], dtype=np.uint64)), b"form"),
        (dict(par=np.array([4, 0, 0, 2], dtype=np.uint64)), b"states"),
        (dict(par=np.array([4, 0, 3, 1 << 11], dtype=np.uint64)), b"aft"),
        (mark_args(code=[push, end0]), b"exactly two predicates"),
        (mark_args(code=[push, end0, push, end1, push, (pred.P_END | (2 << 8), 0)]), b"exactly two predicates"),
        (mark_args(code=[push, end0, push, (pred.P_END, 0)]), b"END k out of order"),
        (mark_args(code=[push, end0, (pred.P_LEAF_CONST | (4 << 8) | (1 << 22), 0), end1]), b"field outside the state"),
        (mark_args(code=[push, end0, push, (15, 0)]), b"unknown opcode"),
        (dict(deg=np.array([1, 0, 3], dtype=np.uint64)), b"out-degrees"),
        (dict(deg=np.array([1, 0, 1], dtype=np.uint64)), b"do not sum"),
        (dict(edges=np.array([1, 0, 3], dtype=np.uint64)), b"target is not a state"),
        (dict(level=np.array([1, 0, 2], dtype=np.uint64)), b"level"),
        (dict(alive=np.array([1, 2, 0], dtype=np.uint64)), b"alive_in"),
        (dict(out=np.zeros(7, dtype=np.uint64)), b"three sections"),
        (dict(res=np.zeros(4, dtype=np.uint64)), b"res of 5 words"),
    ]
    for over, why in bad:
        assert call_mark(good, **over) == -22, why
        assert why in lib.kc_last_error(), (why, lib.kc_last_error())
