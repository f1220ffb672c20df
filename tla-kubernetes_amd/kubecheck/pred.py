"""User-defined invariants: TLA+-flavoured predicates over KubeAPI.tla's
variables, compiled for one (NC, NP, NS) to the flat program csrc/pred.h runs
(DESIGN.md §4.13).  Pure Python, no GPU and no library.

Three parts, which share the AST and nothing else:

* :func:`parse` turns text into an AST, with quantifiers unrolled over the
  model's processes;
* :func:`evaluate` evaluates an AST on a canonical tuple (the yardstick of the
  tests: it never sees the packed state or the program);
* :func:`compile_invariants` lowers ASTs to 16-byte instructions over the
  packed state's words.

Temporal formulas are two such predicates and a shape:
:func:`parse_temporal` splits P ~> Q, [](P => <>Q), []<>Q and <>Q into (form,
P, Q) and refuses every other shape by name; :func:`compile_temporal` compiles
the pair into one program (END 0 = P, END 1 = Q) for kubecheck.LivenessChecker.

Language
  atoms        pc[a]  op[a]  kind[a]  shouldReconcile[a] (clients)  Len(stack[a])
               a \\in DOMAIN requests      requests[a].op      requests[a].status
               a \\in DOMAIN listRequests  listRequests[a].kind  listRequests[a].status
               Cardinality(listRequests[a].objs)   Cardinality(apiState)
               Cardinality({o \\in apiState : F})  with F a conjunction of
                   o.k = "Secret" | "PVC",  a \\in o.vv,  a \\notin o.vv,
                   "spec" \\in DOMAIN o,  "spec" \\notin DOMAIN o
  comparisons  = # /= < <= =< > >=  between an atom and a constant or two atoms
               of one type; atom \\in {c1, c2, ...}
  constants    "C5" (a label, verb, status or kind by the atom's type),
               defaultInitValue (op, kind), TRUE, FALSE, integers
  connectives  /\\ \\/ ~ => <=> ( ) TRUE FALSE   (<=> binds weakest and does not chain, then
               =>, right associative, then \\/, then /\\)
  quantifiers  \\A x \\in S : e   \\E x \\in S : e   with S one of Clients,
               Controllers, Actors or {"Client", ...}

a is a process name as the traces print it ("Client", or "Client1" when the
model has several) or a bound variable.  A field of an absent record equals
no constant: every comparison on it is FALSE except #, which is ~(=).
Object-valued fields (obj[a], requests[a].obj, the stack's saved object) are
out of scope.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

MAX_INSTR = 128
MAX_INV = 8
MAX_DEPTH = 32

LABELS = ["?", "CStart", "C1", "C10", "C11", "c12", "C13", "C2", "C3", "C8", "C6", "C7", "C4", "C5", "PVCStart",
          "PVCListedPVCs", "PVCHavePVCs", "PVCDone", "APIStart", "DoRequest", "DoReply", "DoListRequest",
          "DoListReply"]
CONSTS: Dict[str, Dict[str, int]] = {
    "label": {n: i for i, n in enumerate(LABELS) if i},
    "verb": {"defaultInitValue": 0, "Create": 1, "Get": 2, "Update": 3, "Delete": 4, "Force": 5},
    "status": {"Pending": 1, "Ok": 2, "Error": 3},
    "kind": {"defaultInitValue": 0, "Secret": 1, "PVC": 2},
    "bool": {"FALSE": 0, "TRUE": 1},
}
# atom kind -> (type, record it is a field of or None, clients only)
ATOM_KINDS = {
    "pc": ("label", None), "op": ("verb", None), "kind": ("kind", None), "sr": ("bool", None),
    "stacklen": ("int", None),
    "rq_present": ("bool", None), "rq_op": ("verb", "rq"), "rq_status": ("status", "rq"),
    "lr_present": ("bool", None), "lr_kind": ("kind", "lr"), "lr_status": ("status", "lr"),
    "lr_card": ("int", "lr"),
    "api_card": ("int", None),
}
CMP_OPS = ("=", "#", "<", "<=", ">", ">=")
_FLIP = {"=": "=", "#": "#", "<": ">", "<=": ">=", ">": "<", ">=": "<="}
GHOST = 1 << 63


class PredError(ValueError):
    """A predicate that cannot be parsed, typed or compiled for the model."""


# ------------------------------------------------------------------ the model
def proc_names(nc: int, np: int, ns: int) -> List[str]:
    """ProcSet in tuple order, named as the traces print them."""
    out = []
    for base, cnt in (("Client", nc), ("PVCController", np), ("Server", ns)):
        out += [base if cnt == 1 else f"{base}{i + 1}" for i in range(cnt)]
    return out


def universe_mask(nc: int, np: int, kind: Optional[str] = None, spec: Optional[bool] = None,
                  readers: Sequence[int] = (), non_readers: Sequence[int] = ()) -> int:
    """The elements u = id << (A+1) | spec << A | vv of the object universe that pass the filter."""
    A = nc + np
    m = 0
    for u in range(1 << (A + 2)):
        ident, sp, vv = (u >> (A + 1)) & 1, (u >> A) & 1, u & ((1 << A) - 1)
        if kind is not None and ident != (0 if kind == "Secret" else 1):
            continue
        if spec is not None and sp != int(spec):
            continue
        if any(not (vv >> a) & 1 for a in readers) or any((vv >> a) & 1 for a in non_readers):
            continue
        m |= 1 << u
    return m


def atoms(nc: int, np: int, ns: int) -> List[tuple]:
    """Every atom of the model but the filtered cardinalities: ("atom", kind, actor) / ("atom", "api_card", mask)."""
    out = []
    for a in range(nc + np):
        for k in ATOM_KINDS:
            if k == "api_card" or (k == "sr" and a >= nc):
                continue
            out.append(("atom", k, a))
    out.append(("atom", "api_card", universe_mask(nc, np)))
    return out


def atom_type(atom: tuple) -> str:
    return ATOM_KINDS[atom[1]][0]


# ------------------------------------------------------------------ the parser
_TOKEN = re.compile(r"""\s*(?:
    (?P<str>"[^"]*") | (?P<int>\d+) | (?P<id>[A-Za-z_][A-Za-z0-9_]*) |
    (?P<op><=>|=>|/\\|\\/|\\in\b|\\notin\b|\\A\b|\\E\b|\\lnot\b|\\land\b|\\lor\b|\\neg\b|/=|<=|=<|>=|[~=\#<>:()\[\]{},.])
)""", re.X)


def _tokens(text: str) -> List[Tuple[str, str]]:
    out, pos = [], 0
    text = re.sub(r"\\\*[^\n]*", " ", text)          # \* comments
    while True:
        m = _TOKEN.match(text, pos)
        if not m:
            if text[pos:].strip():
                raise PredError(f"cannot read {text[pos:].strip()[:20]!r}")
            return out
        pos = m.end()
        kind = m.lastgroup
        val = m.group(kind)
        if kind == "op":
            val = {"\\lnot": "~", "\\neg": "~", "\\land": "/\\", "\\lor": "\\/", "/=": "#", "=<": "<="}.get(val, val)
        out.append((kind, val))


class _Parser:
    def __init__(self, text: str, nc: int, np: int, ns: int):
        self.t = _tokens(text)
        self.i = 0
        self.nc, self.np, self.ns = nc, np, ns
        self.A = nc + np
        self.names = proc_names(nc, np, ns)
        self.env: Dict[str, int] = {}

    # -- token helpers
    def peek(self, k: int = 0) -> Tuple[str, str]:
        return self.t[self.i + k] if self.i + k < len(self.t) else ("end", "")

    def at(self, val: str, k: int = 0) -> bool:
        kind, v = self.peek(k)
        return kind in ("op", "id") and v == val

    def take(self, val: str) -> None:
        if not self.at(val):
            raise PredError(f"expected {val!r}, found {self.peek()[1] or 'the end'!r}")
        self.i += 1

    def accept(self, val: str) -> bool:
        if self.at(val):
            self.i += 1
            return True
        return False

    # -- processes
    def actor_of(self, name: str) -> int:
        if name not in self.names:
            raise PredError(f"the model (nc={self.nc}, np={self.np}, ns={self.ns}) has no process {name!r} "
                            f"(it has {', '.join(self.names)})")
        p = self.names.index(name)
        if p >= self.A:
            raise PredError(f"{name!r} is a server: servers hold no state a predicate can read")
        return p

    def proc(self) -> int:
        kind, v = self.peek()
        if kind == "str":
            self.i += 1
            return self.actor_of(v[1:-1])
        if kind == "id" and v in self.env:
            self.i += 1
            return self.env[v]
        raise PredError(f"expected a process name or a bound variable, found {v or 'the end'!r}")

    def is_proc(self, k: int = 0) -> bool:
        kind, v = self.peek(k)
        return (kind == "str" and v[1:-1] in self.names) or (kind == "id" and v in self.env)

    def proc_set(self) -> List[int]:
        kind, v = self.peek()
        if kind == "id" and v in ("Clients", "Controllers", "Actors"):
            self.i += 1
            s = {"Clients": list(range(self.nc)), "Controllers": list(range(self.nc, self.A)),
                 "Actors": list(range(self.A))}[v]
            if not s:
                raise PredError(f"the model (nc={self.nc}, np={self.np}, ns={self.ns}) has no {v}")
            return s
        if self.accept("{"):
            s = [self.proc()]
            while self.accept(","):
                s.append(self.proc())
            self.take("}")
            return s
        raise PredError(f"expected Clients, Controllers, Actors or a set of process names, found {v or 'the end'!r}")

    # -- expressions
    def expr(self):
        if self.at("/\\") or self.at("\\/"):      # a leading bullet
            self.i += 1
        a = self.impl()
        if self.accept("<=>"):             # weakest, and not associative: one per (parenthesised) expression
            return ("iff", a, self.impl())
        return a

    def impl(self):
        a = self.disj()
        if self.accept("=>"):
            return ("implies", a, self.impl())
        return a

    def disj(self):
        a = self.conj()
        while self.accept("\\/"):
            a = ("or", a, self.conj())
        return a

    def conj(self):
        a = self.neg()
        while self.accept("/\\"):
            a = ("and", a, self.neg())
        return a

    def quant(self):
        forall = self.peek()[1] == "\\A"
        self.i += 1
        kind, var = self.peek()
        if kind != "id":
            raise PredError(f"expected a variable after the quantifier, found {var or 'the end'!r}")
        self.i += 1
        self.take("\\in")
        procs = self.proc_set()
        self.take(":")
        start, shadowed = self.i, self.env.get(var)
        out = None
        for p in procs:                          # unrolled: the body parsed once per process
            self.i = start
            self.env[var] = p
            body = self.expr()
            out = body if out is None else (("and" if forall else "or"), out, body)
        if shadowed is None:
            del self.env[var]
        else:
            self.env[var] = shadowed
        return out

    def neg(self):
        if self.accept("~"):
            return ("not", self.neg())
        if self.at("\\A") or self.at("\\E"):
            return self.quant()
        return self.cmp()

    def cmp(self):
        if (self.is_proc() or self.peek()[0] == "str") and (self.at("\\in", 1) or self.at("\\notin", 1)) \
                and self.at("DOMAIN", 2):
            p = self.proc()
            negated = self.peek()[1] == "\\notin"
            self.i += 2
            kind, v = self.peek()
            if v not in ("requests", "listRequests"):
                raise PredError(f"DOMAIN of requests or listRequests, not {v!r}")
            self.i += 1
            a = ("atom", "rq_present" if v == "requests" else "lr_present", p)
            return ("not", a) if negated else a
        lhs = self.term()
        kind, v = self.peek()
        if kind == "op" and v in CMP_OPS:
            self.i += 1
            return self.typed_cmp(v, lhs, self.term())
        if self.accept("\\in") or self.at("\\notin"):
            negated = self.accept("\\notin")
            if lhs[0] != "atom":
                raise PredError("the left side of \\in is an atom")
            self.take("{")
            vals = [self.term()]
            while self.accept(","):
                vals.append(self.term())
            self.take("}")
            e = ("in", lhs, sorted({self.const_value(c, atom_type(lhs)) for c in vals}))
            return ("not", e) if negated else e
        if lhs[0] == "atom":
            if atom_type(lhs) != "bool":
                raise PredError(f"wrong type: {self.show(lhs)} is a {atom_type(lhs)}, not a BOOLEAN")
            return lhs
        if lhs[0] == "rawconst":
            if lhs[1] in ("TRUE", "FALSE"):
                return ("const", lhs[1] == "TRUE")
            raise PredError(f"wrong type: the constant {lhs[1]} is no predicate")
        return lhs

    def term(self):
        kind, v = self.peek()
        if kind == "int":
            self.i += 1
            return ("rawconst", int(v))
        if kind == "str":
            self.i += 1
            return ("rawconst", v[1:-1])
        if kind == "id" and v in ("TRUE", "FALSE", "defaultInitValue"):
            self.i += 1
            return ("rawconst", v)
        if self.accept("("):
            e = self.expr()
            self.take(")")
            return e
        if kind == "id" and v in ("pc", "op", "kind", "shouldReconcile"):
            self.i += 1
            self.take("[")
            p = self.proc()
            self.take("]")
            if v == "shouldReconcile" and p >= self.nc:
                raise PredError(f"shouldReconcile is defined on clients only, not on {self.names[p]!r}")
            return ("atom", "sr" if v == "shouldReconcile" else v, p)
        if kind == "id" and v in ("requests", "listRequests"):
            self.i += 1
            self.take("[")
            p = self.proc()
            self.take("]")
            self.take(".")
            fk, f = self.peek()
            self.i += 1
            ok = {"requests": {"op": "rq_op", "status": "rq_status"},
                  "listRequests": {"kind": "lr_kind", "status": "lr_status"}}[v]
            if f in ("obj", "objs"):
                raise PredError(f"{v}[..].{f} is object-valued: out of scope (Cardinality(listRequests[a].objs) is not)")
            if f not in ok:
                raise PredError(f"unknown name: {v}[..] has no field {f!r}")
            return ("atom", ok[f], p)
        if kind == "id" and v == "Len":
            self.i += 1
            self.take("(")
            self.take("stack")
            self.take("[")
            p = self.proc()
            self.take("]")
            self.take(")")
            return ("atom", "stacklen", p)
        if kind == "id" and v == "Cardinality":
            self.i += 1
            self.take("(")
            a = self.cardinality()
            self.take(")")
            return a
        if kind == "id" and v in ("obj", "stack"):
            raise PredError(f"{v}[..] is object-valued: out of scope")
        if kind == "id":
            raise PredError(f"unknown name {v!r}")
        raise PredError(f"expected an atom or a constant, found {v or 'the end'!r}")

    def cardinality(self):
        if self.accept("apiState"):
            return ("atom", "api_card", universe_mask(self.nc, self.np))
        if self.accept("listRequests"):
            self.take("[")
            p = self.proc()
            self.take("]")
            self.take(".")
            self.take("objs")
            return ("atom", "lr_card", p)
        self.take("{")
        kind, var = self.peek()
        if kind != "id":
            raise PredError("expected {o \\in apiState : F}")
        self.i += 1
        self.take("\\in")
        self.take("apiState")
        self.take(":")
        f = dict(kind=None, spec=None, readers=[], non_readers=[])
        self.accept("/\\")
        while True:
            paren = self.accept("(")
            if self.accept("TRUE"):
                pass
            elif self.at(var):
                self.i += 1
                self.take(".")
                self.take("k")
                self.take("=")
                k, s = self.peek()
                if k != "str" or s[1:-1] not in ("Secret", "PVC"):
                    raise PredError(f'wrong type: o.k is "Secret" or "PVC", not {s}')
                self.i += 1
                f["kind"] = s[1:-1]
            elif self.peek() == ("str", '"spec"'):
                self.i += 1
                neg = not self.accept("\\in")
                if neg:
                    self.take("\\notin")
                self.take("DOMAIN")
                self.take(var)
                f["spec"] = not neg
            else:
                p = self.proc()
                neg = not self.accept("\\in")
                if neg:
                    self.take("\\notin")
                self.take(var)
                self.take(".")
                self.take("vv")
                f["non_readers" if neg else "readers"].append(p)
            if paren:
                self.take(")")
            if not self.accept("/\\"):
                break
        self.take("}")
        return ("atom", "api_card", universe_mask(self.nc, self.np, **f))

    # -- typing
    def show(self, atom) -> str:
        return f"{atom[1]}[{self.names[atom[2]]}]" if atom[1] != "api_card" else "Cardinality(...)"

    def const_value(self, c, typ: str) -> int:
        if c[0] != "rawconst":
            raise PredError("expected a constant")
        v = c[1]
        if typ == "int":
            if not isinstance(v, int):
                raise PredError(f"wrong type: {v!r} compared with an integer")
            return v
        if isinstance(v, int) or v not in CONSTS[typ]:
            raise PredError(f"wrong type: {v!r} is no {typ} (one of {', '.join(CONSTS[typ])})")
        return CONSTS[typ][v]

    def typed_cmp(self, op: str, lhs, rhs):
        if lhs[0] == "rawconst" and rhs[0] == "atom":
            lhs, rhs, op = rhs, lhs, _FLIP[op]
        if lhs[0] != "atom":
            raise PredError("a comparison has an atom on one side at least")
        typ = atom_type(lhs)
        if op not in ("=", "#") and typ != "int":
            raise PredError(f"wrong type: {op} orders integers, and {self.show(lhs)} is a {typ}")
        if rhs[0] == "atom":
            if atom_type(rhs) != typ:
                raise PredError(f"wrong type: {self.show(lhs)} is a {typ}, {self.show(rhs)} a {atom_type(rhs)}")
            return ("cmp", op, lhs, rhs)
        return ("cmp", op, lhs, ("const", self.const_value(rhs, typ)))


def parse(text: str, nc: int = 1, np: int = 1, ns: int = 1):
    """The AST of one predicate for the model (nc, np, ns).

    Nodes: ("const", bool), ("not", e), ("and" | "or" | "implies" | "iff", a, b),
    ("atom", kind, actor) (a BOOLEAN atom), ("cmp", op, atom, atom | ("const", int)),
    ("in", atom, [int, ...]).  Quantifiers are unrolled into and / or chains."""
    p = _Parser(text, nc, np, ns)
    if not p.t:
        raise PredError("empty predicate")
    e = p.expr()
    if p.i != len(p.t):
        raise PredError(f"unexpected {p.peek()[1]!r}")
    if e[0] == "rawconst":
        raise PredError(f"wrong type: the constant {e[1]} is no predicate")
    return e


def parse_definitions(text: str) -> Dict[str, str]:
    """`Name == expr` definitions, in order; an expression runs to the next `Name ==` line.
    Module headers and rules (----, ====) and \\* comments are skipped."""
    defs: Dict[str, str] = {}
    name = None
    for line in text.splitlines():
        line = re.sub(r"\\\*.*", "", line).rstrip()
        if re.match(r"^\s*(-{4,}.*|={4,}|EXTENDS\b.*|VARIABLES?\b.*|CONSTANTS?\b.*)$", line):
            continue
        m = re.match(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s*==(.*)$", line)
        if m:
            name = m.group(1)
            if name in defs:
                raise PredError(f"{name} is defined twice")
            defs[name] = m.group(2)
        elif line.strip():
            if name is None:
                raise PredError(f"text before the first `Name ==` definition: {line.strip()[:30]!r}")
            defs[name] += "\n" + line
    for k, v in defs.items():
        if not v.strip():
            raise PredError(f"{k} has no expression")
    return defs


# ---------------------------------------------------------- temporal formulas
# A formula is two state predicates and one of three shapes:
#   P ~> Q, [](P => <>Q)   form 0, trigger P
#   []<>Q                  form 0, trigger TRUE
#   <>Q                    form 1, trigger = the Init states
# The split works on the text, outside (), [], {} and strings; the operands go
# to parse().  `[]` next to pc["Client"] is no problem: the box is `[` directly
# followed by `]`, which the predicate language never writes.
_SHAPES = "P ~> Q, [](P => <>Q), []<>Q or <>Q over state predicates P, Q"


def _scan_temporal(text: str) -> List[Tuple[int, str, int]]:
    """(position, operator, nesting depth) of every ~>, <> and [] outside strings."""
    out, depth, i = [], 0, 0
    while i < len(text):
        c = text[i]
        if c == '"':
            j = text.find('"', i + 1)
            if j < 0:
                raise PredError("a string without its closing quote")
            i = j + 1
            continue
        if text[i:i + 2] in ("~>", "<>", "[]"):
            out.append((i, text[i:i + 2], depth))
            i += 2
            continue
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth < 0:
                raise PredError(f"unbalanced {c!r}")
        i += 1
    if depth:
        raise PredError("unbalanced brackets")
    return out


def _top_level(text: str, what: Sequence[str]) -> int:
    """The position of the first of `what` at nesting depth 0 outside strings, or -1."""
    depth, i = 0, 0
    while i < len(text):
        c = text[i]
        if c == '"':
            i = text.find('"', i + 1) + 1 or len(text)
            continue
        if depth == 0 and any(text.startswith(w, i) for w in what):
            return i
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        i += 1
    return -1


def _strip_parens(text: str) -> str:
    """text without the parentheses that enclose all of it."""
    text = text.strip()
    while text.startswith("("):
        depth, i, close = 0, 0, -1
        while i < len(text):
            c = text[i]
            if c == '"':
                i = text.find('"', i + 1) + 1 or len(text)
                continue
            if c in "([{":
                depth += 1
            elif c in ")]}":
                depth -= 1
                if depth == 0:
                    close = i
                    break
            i += 1
        if close != len(text) - 1:
            break
        text = text[1:-1].strip()
    return text


def _temporal_operand(text: str, of: str, prefix: bool) -> str:
    """An operand of the temporal operator `of`: it holds no temporal operator,
    and where TLA+'s precedences would read it differently from the way it is
    split here (a prefix operator binds tighter than every connective, ~> looser
    than /\\ and \\/ but tighter than =>) it must be parenthesised."""
    s = text.strip()
    if not s:
        raise PredError(f"{of} lacks an operand")
    inner = _scan_temporal(s)
    if inner:
        _, op, depth = inner[0]
        if depth == 0:
            raise PredError(f"more than one temporal operator ({op} in an operand of {of}): a formula is {_SHAPES}")
        raise PredError(f"the temporal operator {op} inside an operand of {of}: nested temporal formulas are not "
                        f"supported; a formula is {_SHAPES}")
    connectives = ("/\\", "\\/", "=>", "<=>", "\\land", "\\lor") if prefix else ("=>", "<=>")
    if _strip_parens(s) == s and _top_level(s, connectives) >= 0:
        raise PredError(f"parenthesise the operand of {of}: {s[:30]!r} has a connective that binds "
                        f"{'looser' if prefix else 'no tighter'} than {of}")
    return s


def parse_temporal(text: str, nc: int = 1, np: int = 1, ns: int = 1):
    """(form, P_ast, Q_ast) of a temporal formula for the model (nc, np, ns):
    form 0 for P ~> Q, [](P => <>Q) and []<>Q (P = TRUE), form 1 for <>Q (P =
    TRUE; the trigger is the Init states).  Raises PredError, naming what it
    saw, for <>[]Q, a bare []P, more than one temporal operator, a temporal
    operator inside an operand and a text with no temporal operator."""
    body = _strip_parens(re.sub(r"\\\*[^\n]*", " ", text))
    if not body:
        raise PredError("empty formula")
    ops = _scan_temporal(body)
    if not ops:
        raise PredError(f"no temporal operator in {body[:30]!r}: a state predicate: list it under INVARIANT")
    true = ("const", True)

    def sub(s):
        return parse(s, nc, np, ns)

    if body.startswith("[]"):
        rest = body[2:].lstrip()
        if rest.startswith("<>"):
            return 0, true, sub(_temporal_operand(rest[2:], "[]<>", True))
        inner = _strip_parens(rest)
        if not _scan_temporal(inner):
            _temporal_operand(rest, "[]", True)
            raise PredError(f"[]P with a state predicate P ({inner[:30]!r}) is an invariant: list P under INVARIANT")
        if inner == rest.strip():
            raise PredError(f"[] over an unparenthesised temporal formula ({rest[:30]!r}): combined temporal "
                            f"formulas are not supported; a formula is {_SHAPES}")
        at = _top_level(inner, ("=>", "<=>"))
        rhs = inner[at + 2:].lstrip() if at >= 0 and not inner.startswith("<=>", at) else ""
        if at >= 0 and rhs.startswith("<>") and not (at and inner[at - 1] == "<"):
            if rhs[2:].lstrip().startswith("[]"):
                raise PredError(f"<>[]Q under [] ({rhs[:30]!r}): nested temporal formulas are not supported")
            return 0, sub(_temporal_operand(inner[:at], "[](P => <>Q)", False)), \
                sub(_temporal_operand(rhs[2:], "[](P => <>Q)", True))
        raise PredError(f"[] over {inner[:30]!r}: neither P => <>Q nor a state predicate; nested or combined "
                        f"temporal formulas are not supported; a formula is {_SHAPES}")
    if body.startswith("<>"):
        rest = body[2:].lstrip()
        if rest.startswith("[]"):
            raise PredError("<>[]Q (eventually always) is not a stay-set question: it needs an acceptance condition "
                            f"on the SCCs of the whole graph; a formula is {_SHAPES}")
        return 1, true, sub(_temporal_operand(rest, "<>", True))
    top = [o for o in ops if o[1] == "~>" and o[2] == 0]
    if len(top) > 1:
        raise PredError(f"more than one temporal operator (~> twice): a formula is {_SHAPES}")
    if not top:
        _, op, depth = ops[0]
        where = "inside an operand" if depth else "combined with a connective"
        raise PredError(f"the temporal operator {op} {where} in {body[:30]!r}: nested or combined temporal formulas "
                        f"are not supported; a formula is {_SHAPES}")
    at = top[0][0]
    return 0, sub(_temporal_operand(body[:at], "~>", False)), sub(_temporal_operand(body[at + 2:], "~>", False))


def has_temporal(text: str) -> bool:
    """Does the text hold a temporal operator (~>, <>, []) outside strings?"""
    return bool(_scan_temporal(re.sub(r"\\\*[^\n]*", " ", text)))


# ----------------------------------------------------------- direct evaluation
_TUPLE_PER_PROC = 19
_TUPLE_FIELD = {"pc": 0, "op": 1, "kind": 3, "sr": 4, "stacklen": 5, "rq_present": 11, "rq_op": 12,
                "rq_status": 13, "lr_present": 15, "lr_kind": 16, "lr_status": 17}


def _atom_value(atom, t, actors: int) -> Optional[int]:
    """The atom's value on canonical tuple t, or None for a field of an absent record.
    Bit 63 of word 0 is the lostUpdate ghost only while the object universe has
    fewer than 64 elements; with four actors it is the object u = 63."""
    _, kind, a = atom
    if kind == "api_card":
        api = int(t[0]) if actors >= 4 else int(t[0]) & ~GHOST
        return bin(api & a).count("1")
    q = 1 + _TUPLE_PER_PROC * a
    rec = ATOM_KINDS[kind][1]
    if rec == "rq" and not int(t[q + 11]):
        return None
    if rec == "lr" and not int(t[q + 15]):
        return None
    if kind == "lr_card":
        return bin(int(t[q + 18])).count("1")
    return int(t[q + _TUPLE_FIELD[kind]])


def evaluate(ast, t, nc: int = 1, np: int = 1, ns: int = 1) -> bool:
    """The predicate's value on one canonical tuple (include/kubecheck.h: word 0 apiState, 19 words per process)."""
    k = ast[0]
    if k == "const":
        return bool(ast[1])
    if k == "not":
        return not evaluate(ast[1], t, nc, np, ns)
    if k == "and":
        return evaluate(ast[1], t, nc, np, ns) and evaluate(ast[2], t, nc, np, ns)
    if k == "or":
        return evaluate(ast[1], t, nc, np, ns) or evaluate(ast[2], t, nc, np, ns)
    if k == "implies":
        return (not evaluate(ast[1], t, nc, np, ns)) or evaluate(ast[2], t, nc, np, ns)
    if k == "iff":
        return evaluate(ast[1], t, nc, np, ns) == evaluate(ast[2], t, nc, np, ns)
    if k == "atom":
        return bool(_atom_value(ast, t, nc + np))
    if k == "in":
        v = _atom_value(ast[1], t, nc + np)
        return v is not None and v in ast[2]
    if k == "cmp":
        _, op, lhs, rhs = ast
        a = _atom_value(lhs, t, nc + np)
        b = rhs[1] if rhs[0] == "const" else _atom_value(rhs, t, nc + np)
        if a is None or b is None:
            return op == "#"
        return {"=": a == b, "#": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
    raise PredError(f"bad AST node {k!r}")


# ------------------------------------------------------------------ the compiler
P_LEAF_CONST, P_LEAF_SET, P_LEAF_FIELD, P_LEAF_POPC, P_PUSH, P_AND, P_OR, P_NOT, P_END = range(9)
_CMP_CODE = {"=": 0, "#": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}


class Layout:
    """Where the packed state (csrc/kubeapi_spec.h Model<NC, NP, NS>) keeps each atom."""

    def __init__(self, nc: int, np: int, ns: int):
        A = nc + np
        if not 1 <= A <= 4:
            raise PredError("a model has 1 to 4 actors")
        self.nc, self.np, self.ns, self.A = nc, np, ns, A
        self.U = 1 << (A + 2)
        objb = (3 + self.U - 1).bit_length()          # ceil(log2(3 + U))
        self.per_word = 64 // self.U
        obj_words = (A + self.per_word - 1) // self.per_word
        self.W = (1 + A + obj_words + 1) & ~1
        off, f = 0, {}
        for name, bits in (("pc", 5), ("rq_present", 1), ("rq_status", 2), ("rq_op", 3), ("rq_obj", objb),
                           ("lr_present", 1), ("lr_status", 2), ("lr_kind", 2), ("stacklen", 1), ("sproc", 2),
                           ("sret", 5), ("sop", 3), ("sobj", objb), ("skind", 2), ("op", 3), ("obj", objb),
                           ("kind", 2), ("sr", 1)):
            f[name] = (off, bits)
            off += bits
        assert off <= 64
        self.fields = f

    def field(self, atom) -> Tuple[int, int, int]:
        """(word, shift, width) of a field atom."""
        _, kind, a = atom
        if kind == "lr_card":
            return (1 + self.A + a // self.per_word, (a % self.per_word) * self.U, self.U)
        off, bits = self.fields[kind]
        return (1 + a, off, bits)


def _atom_max(atom, lay: Layout) -> int:
    if atom[1] == "stacklen":
        return 1
    if atom[1] == "lr_card":
        return lay.U
    return bin(atom[2]).count("1")


class _Emitter:
    def __init__(self, lay: Layout):
        self.lay = lay
        self.code: List[Tuple[int, int]] = []
        self.depth = self.max_depth = 0

    def emit(self, hdr: int, opnd: int = 0, push: int = 0) -> None:
        self.code.append((hdr, opnd & (2 ** 64 - 1)))
        self.depth += push
        self.max_depth = max(self.max_depth, self.depth)

    @staticmethod
    def fbits(word: int, shift: int, width: int) -> int:
        return (word << 8) | (shift << 16) | (width << 22)

    def push_const(self, b: bool) -> None:
        self.emit(P_PUSH, int(b), 1)

    def guard(self, atom) -> bool:
        """Push `the atom's record is present`; False when the atom is no record field."""
        rec = ATOM_KINDS[atom[1]][1]
        if rec is None:
            return False
        w, s, n = self.lay.field(("atom", rec + "_present", atom[2]))
        self.emit(P_LEAF_CONST | self.fbits(w, s, n), 1, 1)
        return True

    def atom_const(self, op: str, atom, c: int) -> None:
        """Push atom op c (op is not #)."""
        g = self.guard(atom)
        if atom[1] in ("api_card", "lr_card"):
            if atom[1] == "api_card":
                word, mask = 0, atom[2]
            else:
                word, shift, width = self.lay.field(atom)
                mask = ((1 << width) - 1) << shift
            if c > 64:                     # a popcount is at most 64
                self.push_const(op in ("<", "<="))
            else:
                self.emit(P_LEAF_POPC | (_CMP_CODE[op] << 4) | (word << 8) | (c << 32), mask, 1)
        else:
            w, s, n = self.lay.field(atom)
            self.emit(P_LEAF_CONST | (_CMP_CODE[op] << 4) | self.fbits(w, s, n), c, 1)
        if g:
            self.emit(P_AND, push=-1)

    def atom_atom(self, op: str, lhs, rhs) -> None:
        """Push lhs op rhs (op is not #)."""
        cards = ("api_card", "lr_card")
        if lhs[1] not in cards and rhs[1] not in cards:
            gl, gr = self.guard(lhs), self.guard(rhs)
            (w, s, n), (w2, s2, n2) = self.lay.field(lhs), self.lay.field(rhs)
            self.emit(P_LEAF_FIELD | (_CMP_CODE[op] << 4) | self.fbits(w, s, n) | (self.fbits(w2, s2, n2) << 24), 0, 1)
            for g in (gl, gr):
                if g:
                    self.emit(P_AND, push=-1)
            return
        # a cardinality has no field to compare: enumerate the side with the
        # smaller range,  \/ v : E = v /\ other op' v
        if _atom_max(lhs, self.lay) <= _atom_max(rhs, self.lay):
            e, other, oop = lhs, rhs, _FLIP[op]          # lhs = v  =>  rhs flip(op) v
        else:
            e, other, oop = rhs, lhs, op
        for v in range(_atom_max(e, self.lay) + 1):
            self.atom_const("=", e, v)
            self.atom_const(oop, other, v)
            self.emit(P_AND, push=-1)
            if v:
                self.emit(P_OR, push=-1)

    def node(self, ast) -> None:
        k = ast[0]
        if k == "const":
            self.push_const(ast[1])
        elif k == "not":
            self.node(ast[1])
            self.emit(P_NOT)
        elif k in ("and", "or"):
            self.node(ast[1])
            self.node(ast[2])
            self.emit(P_AND if k == "and" else P_OR, push=-1)
        elif k == "implies":
            self.node(ast[1])
            self.emit(P_NOT)
            self.node(ast[2])
            self.emit(P_OR, push=-1)
        elif k == "iff":                   # (a /\ b) \/ (~a /\ ~b)
            self.node(("or", ("and", ast[1], ast[2]), ("and", ("not", ast[1]), ("not", ast[2]))))
        elif k == "atom":
            self.atom_const("=", ast, 1)
        elif k == "in":
            atom, vals = ast[1], ast[2]
            if atom[1] in ("api_card", "lr_card"):
                if not vals:
                    self.push_const(False)
                for j, v in enumerate(vals):
                    self.atom_const("=", atom, v)
                    if j:
                        self.emit(P_OR, push=-1)
            else:
                g = self.guard(atom)
                w, s, n = self.lay.field(atom)
                self.emit(P_LEAF_SET | self.fbits(w, s, n), sum(1 << v for v in vals if v < 64), 1)
                if g:
                    self.emit(P_AND, push=-1)
        elif k == "cmp":
            _, op, lhs, rhs = ast
            neg = op == "#"
            op = "=" if neg else op
            if rhs[0] == "const":
                self.atom_const(op, lhs, rhs[1])
            else:
                self.atom_atom(op, lhs, rhs)
            if neg:
                self.emit(P_NOT)
        else:
            raise PredError(f"bad AST node {k!r}")


class Program:
    """A compiled set of invariants: `words` is 2 * n_instr uint64 values (hdr, opnd per instruction)."""

    def __init__(self, names: List[str], code: List[Tuple[int, int]], depth: int, lay: Layout):
        self.names = names
        self.code = code
        self.n_instr = len(code)
        self.depth = depth
        self.W = lay.W
        self.words = [x for ins in code for x in ins]

    def array(self):
        import numpy
        return numpy.array(self.words, dtype=numpy.uint64)


def compile_invariants(invariants, nc: int = 1, np: int = 1, ns: int = 1) -> Program:
    """Compile {name: text or AST} (or a list of texts / ASTs) into one program; invariant k is the k-th given."""
    if not isinstance(invariants, dict):
        invariants = {f"Inv{k}": e for k, e in enumerate(invariants)}
    if not invariants:
        raise PredError("no invariant given")
    if len(invariants) > MAX_INV:
        raise PredError(f"{len(invariants)} invariants: at most {MAX_INV} in one run")
    lay = Layout(nc, np, ns)
    em = _Emitter(lay)
    for k, (name, e) in enumerate(invariants.items()):
        try:
            ast = parse(e, nc, np, ns) if isinstance(e, str) else e
            em.node(ast)
        except PredError as err:
            raise PredError(f"{name}: {err}") from None
        em.emit(P_END | (k << 8), push=-1)
        if em.max_depth > MAX_DEPTH:
            raise PredError(f"{name}: nesting depth {em.max_depth}: at most {MAX_DEPTH} (parenthesise to the left, "
                            "or split the invariant)")
        if len(em.code) > MAX_INSTR:
            raise PredError(f"{name}: the program reaches {len(em.code)} instructions: at most {MAX_INSTR} over all "
                            "the invariants of a run")
    return Program(list(invariants), em.code, em.max_depth, lay)


def compile_temporal(text: str, nc: int = 1, np: int = 1, ns: int = 1) -> Tuple[int, Program]:
    """(form, program) of a temporal formula (parse_temporal): the program always holds exactly two predicates,
    END 0 = the trigger P ("trigger"; TRUE for []<>Q and <>Q) and END 1 = the goal Q ("goal")."""
    form, p_ast, q_ast = parse_temporal(text, nc, np, ns)
    return form, compile_invariants({"trigger": p_ast, "goal": q_ast}, nc, np, ns)
