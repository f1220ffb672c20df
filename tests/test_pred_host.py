"""User-defined invariants without a GPU: the parser, every error path and
limit of the compiler, the compiled program (kc_pred_eval, the code k_pred
runs) against pred.evaluate on whole state spaces, the host model against its
fixture file, the C entry points' argument checks, and pred.h's host path
under AddressSanitizer and UBSan in a program of its own."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import kubecheck
from kubecheck import pred
from kubecheck.pred import PredError

import pred_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOFAULT = dict(can_fail=False, can_timeout=False)


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


# ------------------------------------------------------------------ the parser
A, B, Cc = (("atom", "sr", 0), ("atom", "rq_present", 0), ("atom", "lr_present", 0))
SR, RQ, LR = 'shouldReconcile["Client"]', '"Client" \\in DOMAIN requests', '"Client" \\in DOMAIN listRequests'


def test_precedence_of_implication_against_conjunction_and_disjunction():
    assert pred.parse(f"{SR} /\\ {RQ} => {LR}") == ("implies", ("and", A, B), Cc)
    assert pred.parse(f"{SR} => {RQ} \\/ {LR}") == ("implies", A, ("or", B, Cc))
    assert pred.parse(f"{SR} \\/ {RQ} /\\ {LR}") == ("or", A, ("and", B, Cc))
    assert pred.parse(f"{SR} => {RQ} => {LR}") == ("implies", A, ("implies", B, Cc))          # right associative
    assert pred.parse(f"~{SR} /\\ {RQ}") == ("and", ("not", A), B)
    assert pred.parse(f"{SR} <=> {RQ} => {LR}") == ("iff", A, ("implies", B, Cc))
    assert pred.parse(f"({SR} => {RQ}) /\\ {LR}") == ("and", ("implies", A, B), Cc)
    assert pred.parse(f"{SR} => {RQ} <=> {LR}") == ("iff", ("implies", A, B), Cc)
    with pytest.raises(PredError, match="unexpected '<=>'"):
        pred.parse(f"{SR} <=> {RQ} <=> {LR}")                                                  # does not chain
    assert pred.parse(f"/\\ {SR}\n/\\ {RQ}") == ("and", A, B)                                  # a bulleted list
    assert pred.parse('pc["Client"] /= "C5"') == pred.parse('pc["Client"] # "C5"') == \
        ("cmp", "#", ("atom", "pc", 0), ("const", 13))
    assert pred.parse('2 >= Cardinality(apiState)') == pred.parse('Cardinality(apiState) =< 2')
    assert pred.parse('pc["Client"] \\in {"C5", "C4", "C5"}') == ("in", ("atom", "pc", 0), [12, 13])


def test_nested_quantifiers_are_unrolled():
    e = pred.parse(r'\A c \in Clients : \E p \in Controllers : pc[c] = "C5" => pc[p] = "PVCDone"', 2, 2, 1)
    leaf = lambda c, p: ("implies", ("cmp", "=", ("atom", "pc", c), ("const", 13)),      # noqa: E731
                         ("cmp", "=", ("atom", "pc", p), ("const", 17)))
    assert e == ("and", ("or", leaf(0, 2), leaf(0, 3)), ("or", leaf(1, 2), leaf(1, 3)))
    # the body runs to the end of the expression, a literal set names processes, a variable may be shadowed
    e = pred.parse(r'\E a \in {"Client2", "PVCController"} : shouldReconcile["Client1"] /\ Len(stack[a]) = 1', 2, 1, 1)
    assert e == ("or", ("and", ("atom", "sr", 0), ("cmp", "=", ("atom", "stacklen", 1), ("const", 1))),
                 ("and", ("atom", "sr", 0), ("cmp", "=", ("atom", "stacklen", 2), ("const", 1))))
    e = pred.parse(r'\A a \in Clients : (\E a \in Controllers : pc[a] = "PVCDone") \/ shouldReconcile[a]', 1, 1, 1)
    assert e == ("or", ("cmp", "=", ("atom", "pc", 1), ("const", 17)), ("atom", "sr", 0))
    assert pred.compile_invariants([r'\A a \in Actors : \A b \in Actors : pc[a] # "C5" \/ pc[b] # "C4"'], 1, 3, 1).n_instr \
        == 16 * 5 + 15 + 1          # 16 bodies of (leaf, NOT, leaf, NOT, OR), 15 ANDs, END


@pytest.mark.parametrize("text,model,words", [
    ('foo["Client"] = 1', (1, 1, 1), "unknown name 'foo'"),
    ('requests["Client"].verb = "Get"', (1, 1, 1), "no field 'verb'"),
    ('requests["Client"].obj = 1', (1, 1, 1), "object-valued"),
    ('obj["Client"] = 1', (1, 1, 1), "object-valued"),
    ('pc["Client"] = "Pending"', (1, 1, 1), "wrong type"),
    ('pc["Client"] = 3', (1, 1, 1), "wrong type"),
    ('pc["Client"] < "C5"', (1, 1, 1), "orders integers"),
    ('pc["Client"] = op["Client"]', (1, 1, 1), "wrong type"),
    ('Len(stack["Client"])', (1, 1, 1), "not a BOOLEAN"),
    ('Cardinality(apiState) = TRUE', (1, 1, 1), "wrong type"),
    ('"C5"', (1, 1, 1), "no predicate"),
    ('pc["Client2"] = "C5"', (1, 1, 1), "has no process 'Client2'"),
    ('pc["Client"] = "C5"', (2, 1, 1), "has no process 'Client'"),
    ('"PVCController" \\in DOMAIN requests', (1, 0, 1), "has no process 'PVCController'"),
    ('pc["Server"] = "APIStart"', (1, 1, 1), "is a server"),
    ('\\A p \\in Controllers : pc[p] = "PVCDone"', (1, 0, 1), "has no Controllers"),
    ('\\A c \\in Clients : shouldReconcile[c]', (0, 1, 1), "has no Clients"),
    ('\\A p \\in Nodes : pc[p] = "C5"', (1, 1, 1), "expected Clients, Controllers, Actors"),
    ('shouldReconcile["PVCController"]', (1, 1, 1), "clients only"),
    ('Cardinality({o \\in apiState : o.k = "Pod"}) = 0', (1, 1, 1), "wrong type"),
    ('pc["Client"] = "C5" /\\', (1, 1, 1), "expected an atom"),
    ('(pc["Client"] = "C5"', (1, 1, 1), "expected ')'"),
    ('pc["Client"] = "C5" )', (1, 1, 1), "unexpected ')'"),
    ('pc["Client"] ? "C5"', (1, 1, 1), "cannot read"),
    ('', (1, 1, 1), "empty"),
])
def test_every_error_path_says_what_is_wrong(text, model, words):
    with pytest.raises(PredError) as e:
        pred.parse(text, *model)
    assert words in str(e.value)


def test_each_limit():
    leaf = 'pc["Client"] = "C5"'
    # 8 invariants pass, 9 do not
    pred.compile_invariants([leaf] * 8)
    with pytest.raises(PredError) as e:
        pred.compile_invariants([leaf] * 9)
    assert "at most 8" in str(e.value)
    # 128 instructions: one leaf + 63 x (leaf, OR) + END = 128 passes, one more does not
    assert pred.compile_invariants([" \\/ ".join([leaf] * 64)]).n_instr == 128
    with pytest.raises(PredError) as e:
        pred.compile_invariants([" \\/ ".join([leaf] * 65)])
    assert "at most 128" in str(e.value)
    with pytest.raises(PredError):
        pred.compile_invariants([" \\/ ".join([leaf] * 33)] * 2)      # over all the invariants of a run
    # nesting: a right-leaning chain of 32 leaves needs 32 stack bits, 33 is one too many
    deep = lambda n: "(".join([leaf + " /\\ "] * (n - 1)) + leaf + ")" * (n - 2)     # noqa: E731
    assert pred.compile_invariants([deep(32)]).depth == 32
    with pytest.raises(PredError) as e:
        pred.compile_invariants([deep(33)])
    assert "at most 32" in str(e.value) and "Inv0" in str(e.value)
    with pytest.raises(PredError):
        pred.compile_invariants({})


def test_c_side_limits_and_argument_checks():
    lib = kubecheck.load()
    cfg = kubecheck.ModelConfig().to_c()
    t = np.ascontiguousarray(kubecheck.Spec(kubecheck.ModelConfig()).init()[0])
    END0 = [pred.P_END, 0]
    leaf = [pred.P_LEAF_CONST | (1 << 8) | (5 << 22), 1]

    def ev(words, n=None):
        w = np.array(words, dtype=np.uint64)
        return lib.kc_pred_eval(C.byref(cfg), u64(w), len(words) // 2 if n is None else n, u64(t))
    assert ev(leaf + END0) in (0, 1)
    bad = [
        ([pred.P_AND, 0] + END0, b"fewer than two"),                          # pops more than was pushed
        (leaf * 33 + [pred.P_AND, 0] * 32 + END0, b"deeper than 32"),
        (leaf + leaf + [pred.P_OR, 0] + END0 + (leaf + END0) * 62 + leaf, b"128"),   # 129 instructions
        ((leaf + [pred.P_END | (0 << 8), 0]) * 2, b"out of order"),
        (sum(([leaf[0], 1, pred.P_END | (k << 8), 0] for k in range(9)), []), b"more than 8"),
        ([pred.P_LEAF_CONST | (4 << 8) | (5 << 22), 1] + END0, b"field outside"),          # word 4 of a 4-word state
        ([pred.P_LEAF_CONST | (1 << 8) | (60 << 16) | (5 << 22), 1] + END0, b"field outside"),   # shift + width > 64
        ([pred.P_LEAF_CONST | (1 << 8), 1] + END0, b"field outside"),                      # width 0
        ([pred.P_LEAF_POPC | (9 << 8), 1] + END0, b"word index"),
        ([pred.P_LEAF_POPC | (65 << 32), 1] + END0, b"0..64"),
        ([15, 0] + END0, b"unknown opcode"),
        ([pred.P_LEAF_CONST | (7 << 4) | (1 << 8) | (5 << 22), 1] + END0, b"compare op"),
        (leaf, b"END"),
        (leaf + leaf + END0, b"other than one bit"),
    ]
    for words, why in bad:
        assert ev(words) == -22 and why in lib.kc_last_error(), why
    assert ev(leaf + END0, 0) == -22
    assert lib.kc_pred_eval(None, None, 0, None) == -22
    t2 = t.copy()
    t2[-19] = 3          # the server's pc is not APIStart: outside the lowered domain
    w = np.array(leaf + END0, dtype=np.uint64)
    assert lib.kc_pred_eval(C.byref(cfg), u64(w), 2, u64(t2)) == -22
    # kc_pred_selftest validates on the host before it looks for a GPU
    st = np.zeros(4, dtype=np.uint64)
    out = np.zeros(8 + 10, dtype=np.uint64)
    assert lib.kc_pred_selftest(4, None, 0, None, 0, 0, None, 0) == -22
    assert lib.kc_pred_selftest(5, u64(w), 2, u64(st), 1, 0, u64(out), len(out)) == -22 and b"4, 6 or 10" in lib.kc_last_error()
    assert lib.kc_pred_selftest(4, u64(w), 2, u64(st), 0, 0, u64(out), len(out)) == -22
    assert lib.kc_pred_selftest(4, u64(w), 2, u64(st), 1, 0, u64(out), 17) == -22
    bw = np.array([pred.P_AND, 0] + END0, dtype=np.uint64)
    assert lib.kc_pred_selftest(4, u64(bw), 2, u64(st), 1, 0, u64(out), len(out)) == -22 and b"bad program" in lib.kc_last_error()
    assert lib.kc_engine_set_invariants(None, u64(w), 2) == -22
    assert lib.kc_engine_invariant_stats(None, u64(out), 9) == -22
    for sym in ("kc_engine_set_invariants", "kc_engine_invariant_stats", "kc_pred_eval", "kc_pred_selftest"):
        assert hasattr(lib, sym)
    assert "pred" in kubecheck.__all__ and kubecheck.pred is pred


# ----------------------------------------------------- compile against evaluate
def states_of(model, **kw):
    out = []
    pred_model.run(*model, on_level=lambda d, ts: out.extend(ts), **kw)
    return np.array(out, dtype=np.uint64)


def random_ast(rng, table, depth):
    if depth == 0 or rng.random() < 0.25:
        a = rng.choice(table)
        typ = pred.atom_type(a)
        kind = rng.random()
        if typ == "bool" and kind < 0.4:
            return a
        if typ == "int":
            top = {"stacklen": 1, "lr_card": 3}.get(a[1], 4)
            if kind < 0.25:
                b = rng.choice([x for x in table if pred.atom_type(x) == "int"])
                return ("cmp", rng.choice(pred.CMP_OPS), a, b)
            if kind < 0.4:
                return ("in", a, sorted(rng.sample(range(top + 2), 2)))
            return ("cmp", rng.choice(pred.CMP_OPS), a, ("const", rng.randrange(top + 2)))
        vals = sorted(set(pred.CONSTS[typ].values()))
        if kind < 0.2:
            b = rng.choice([x for x in table if pred.atom_type(x) == typ])
            return ("cmp", rng.choice("=#"), a, b)
        if kind < 0.4:
            return ("in", a, sorted(rng.sample(vals, min(len(vals), rng.randrange(1, 4)))))
        return ("cmp", rng.choice("=#"), a, ("const", rng.choice(vals)))
    op = rng.choice(["not", "and", "or", "implies", "iff", "and", "or"])
    if op == "not":
        return ("not", random_ast(rng, table, depth - 1))
    return (op, random_ast(rng, table, depth - 1), random_ast(rng, table, depth - 1))


def random_asts(rng, table, n, model, depth=5):
    """n seeded random ASTs that compile on their own (a draw past the instruction or depth limit is drawn again:
    the limits have their own test); most draws do."""
    out, draws = {}, 0
    while len(out) < n:
        a = random_ast(rng, table, rng.randrange(1, depth))
        draws += 1
        try:
            pred.compile_invariants([a], *model)
        except PredError as e:
            assert "at most" in str(e)
            continue
        out[f"R{draws}"] = a
    assert draws <= 2 * n
    return out


def agree(model, tuples, named_asts):
    """kc_pred_eval(program) == pred.evaluate(ast) for every AST on every tuple; programs of up to 8 invariants."""
    lib = kubecheck.load()
    cfg = kubecheck.ModelConfig(nc=model[0], np=model[1], ns=model[2]).to_c()
    items = list(named_asts.items())
    while items:
        batch, n = {}, 0
        while items and len(batch) < 8:            # as many as fit the instruction limit
            k, a = items[0]
            try:
                pred.compile_invariants(dict(batch, **{k: a}), *model)
            except PredError:
                assert batch, f"{k} does not compile on its own"
                break
            batch[k] = a
            items.pop(0)
        prog = pred.compile_invariants(batch, *model)
        words = prog.array()
        asts = list(batch.values())
        for t in tuples:
            got = lib.kc_pred_eval(C.byref(cfg), u64(words), prog.n_instr, u64(t))
            want = sum((not pred.evaluate(a, t, *model)) << k for k, a in enumerate(asts))
            assert got == want, (list(batch), [int(x) for x in t])
        n += len(batch)


SPACES = [((1, 0, 1), {}, 207, pred_model.EXAMPLES_C101),
          ((1, 1, 1), NOFAULT, 8203, pred_model.EXAMPLES_M1),
          ((1, 1, 1), dict(max_levels=21), None, pred_model.EXAMPLES_M1)]       # Model_1, levels 1-20


@pytest.mark.parametrize("model,kw,count,examples", SPACES)
def test_program_equals_evaluate_on_whole_state_spaces(model, kw, count, examples):
    tuples = states_of(model, **kw)
    assert count is None or len(tuples) == count
    asts = {k: pred.parse(v, *model) for k, v in examples.items()}
    assert all(isinstance(pred.evaluate(a, tuples[0], *model), bool) for a in asts.values())
    agree(model, tuples, asts)
    rng = random.Random(20261021 + len(tuples))
    table = pred.atoms(*model) + [("atom", "api_card", pred.universe_mask(model[0], model[1], kind="Secret")),
                                  ("atom", "api_card", pred.universe_mask(model[0], model[1], spec=False, readers=[0]))]
    agree(model, tuples, random_asts(rng, table, 120, model))


def test_np2_examples_compile_and_agree_on_early_levels():
    tuples = states_of((1, 2, 1), max_levels=15)
    agree((1, 2, 1), tuples, {k: pred.parse(v, 1, 2, 1) for k, v in pred_model.EXAMPLES_NP2.items()})
    # four actors: 64 objects fill word 0, and each objs mask has a word of its own
    t4 = states_of((2, 2, 1), max_levels=7)
    rng = random.Random(7)
    agree((2, 2, 1), t4, random_asts(rng, pred.atoms(2, 2, 1), 24, (2, 2, 1), depth=4))


def test_layout_matches_the_library():
    lib = kubecheck.load()
    for model in [(1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 0, 1), (1, 3, 1), (2, 2, 1), (1, 0, 1), (0, 1, 1)]:
        assert pred.Layout(*model).W == lib.kc_spec_state_words(*model)


def test_eval_invariant_and_the_ghost():
    sp = kubecheck.Spec(kubecheck.ModelConfig())
    init = sp.init()
    assert list(sp.eval_invariant('shouldReconcile["Client"]', init)) == [False, True]
    ghost = init.copy()
    ghost[:, 0] |= np.uint64(1 << 63)            # lostUpdate is never part of apiState
    assert list(sp.eval_invariant("Cardinality(apiState) = 0", ghost)) == [True, True]
    assert pred.evaluate(pred.parse("Cardinality(apiState) = 0"), ghost[0])
    # a field of an absent record equals no constant
    for e, want in [('requests["Client"].op = "Get"', False), ('requests["Client"].op # "Get"', True),
                    ('requests["Client"].op \\in {"Get", "Create"}', False),
                    ('Cardinality(listRequests["Client"].objs) = 0', False),
                    ('Cardinality(listRequests["Client"].objs) <= Cardinality(apiState)', False),
                    ('requests["Client"].op = op["Client"]', False)]:
        assert list(sp.eval_invariant(e, init)) == [want, want], e
        assert pred.evaluate(pred.parse(e), init[0]) is want


def test_bit_63_is_an_object_when_there_are_four_actors():
    """With 64 objects u = 63 (the PVC with a spec, read by all four) is bit 63 of word 0, not the ghost."""
    sp = kubecheck.Spec(kubecheck.ModelConfig(nc=2, np=2))
    t = sp.init()[0].copy()
    t[0] = np.uint64((1 << 63) | 1)
    for e, want in [("Cardinality(apiState) = 2", True), ("Cardinality(apiState) = 1", False),
                    ('Cardinality({o \\in apiState : o.k = "PVC" /\\ "PVCController2" \\in o.vv}) = 1', True),
                    ('Cardinality({o \\in apiState : o.k = "Secret"}) = 1', True)]:
        assert pred.evaluate(pred.parse(e, 2, 2, 1), t, 2, 2, 1) is want, e
        assert list(sp.eval_invariant(e, [t])) == [want], e
    # with fewer actors the same bit is the ghost, and counts for nothing
    t3 = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2)).init()[0].copy()
    t3[0] = np.uint64((1 << 63) | 1)
    assert pred.evaluate(pred.parse("Cardinality(apiState) = 1", 1, 2, 1), t3, 1, 2, 1)


# ---------------------------------------------------------- the model's fixtures
def test_fixture_file_is_what_the_model_computes():
    with open(os.path.join(ROOT, "tests", "golden", "pred_fixtures.json")) as f:
        rows = json.load(f)["rows"]
    assert sorted(rows) == sorted(r[0] for r in pred_model.ROWS)
    for rid in pred_model.SMALL:
        assert json.loads(json.dumps(pred_model.row_fixture(rid))) == rows[rid], rid
    levels = {rid: (rows[rid].get("err_level"), list(rows[rid]["violations"].values())) for rid in rows}
    assert levels["model1_store1"] == (9, [1]) and levels["model1_c4"] == (7, [1]) and levels["model1_c5"] == (8, [1])
    assert levels["model1_pvcdone"] == (17, [1]) and levels["model1_onepending"] == (5, [2])
    assert levels["variant2_oov"] == (22, [1]) and levels["variant5_oov"][0] == 1
    assert levels["np2_bothdone"] == (25, [2]) and levels["np2_c5_bothdone"] == (34, [6])
    h = rows["model1_holds"]
    assert (h["generated"], h["distinct"], h["depth"], h["states_evaluated"]) == (577736, 163408, 124, 163408)


def test_model_precedence_rule():
    """A user violation of level L comes before the built-in error the expansion of L finds; the counts are whole-level."""
    fx = pred_model.row_fixture("variant2_precedence")
    plain = pred_model.run(1, 1, 1, variant=2)
    assert plain["error"]["kind"] == "invariant" and plain["error"]["level"] == fx["err_level"] + 1 == 22
    assert fx["verdict"] == "violated" and fx["trace_len"] == 21
    assert fx["level_width"][:21] == plain["level_width"] and len(fx["level_width"]) == 22
    assert fx["generated"] == plain["generated"] and fx["distinct"] == plain["distinct"]


# ------------------------------------------- pred.h's host path under sanitizers
def test_pred_host_path_under_asan_ubsan(tmp_path):
    """csrc/pred_host_check.cpp (its own main, host compiler, no HIP): pred_validate and pred_eval on hand-made words."""
    cxx = "g++"
    exe = str(tmp_path / "pred_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "tla-kubernetes_amd", "csrc"),
                    os.path.join(ROOT, "tla-kubernetes_amd", "csrc", "pred_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pred_host_check: ok" in r.stdout
