"""Host model of the second half of a wide BFS level: the kernels that turn
k_claim's per-parent newmask words into the next frontier (csrc/
engine_kernels.h: the tile scan and its marks, the link emit, the materialising
emit, the rebuild from links, the parent-chain walk, k_claim's tile order).

Written from the contract in the kernels' comments, in plain Python integers
(the *_np variants do the same with numpy, for the sizes the GPU tests run):

  scan    off[t] = sum of tot[0 .. t), off[T] = the total; cells past T do
          not count.
  marks   mark[k] = the prefix at position k * stride for k < nmark, and
          mark[nmark] = the prefix at `extra`; a position past T (or no
          `extra`) leaves its mark alone, position T reads the total.
  emit    the new states of a chunk in (parent, set bit of its newmask) order;
          entry number e goes to index o = chunk_base + e.  The link emit
          writes link[o] = (base + parent) << 8 | position and the trace
          entry parent[next_gidx + o] = level_gidx + base + parent,
          ord[next_gidx + o] = position, only for o < cap, and raises
          DF_CAPACITY iff some o >= cap.  outdeg[min(popcount, 15)] counts
          every parent.
          The materialising emit also stores successor `position` of the
          parent at next[o - next_base], counts its action (act_dist) and its
          own successors (next_cand), and keeps the minimum key (base +
          parent) << 16 | position << 8 | E_INVARIANT over the new states that
          violate an invariant.
  rebuild state i of a deferred frontier = successor `position` of state
          `parent` of the previous frontier, from link[i] or from the trace
          (parent[gidx0 + i] - prev_gidx0, ord[gidx0 + i]); a violation sets
          DF_INVARIANT and defer_inv_n = ~(the lowest violating i).
  chain   out[k] = g_k << 8 | ord[g_k] along g_0 = g, g_{k+1} = parent[g_k],
          until parent = ~0; len = 0 for a chain longer than cap.
  spread  block b of G takes tile (b % S) * (G // S) + min(b % S, G % S) +
          b // S for 0 < S < G, else b: a bijection of [0, G).

Successors, actions, invariants and successor counts come from kubecheck.Spec
(SpecLevel), so the model needs the library but no GPU."""
import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
TILE = 256
CSUM_TILES = 64
EMIT_TPB = 4
OUTDEG_BINS = 16
E_INVARIANT = 2
DF_INVARIANT, DF_CAPACITY = 1, 2
FORE = 8                      # KC_EMIT_FORE: guard elements before every output
K_SCAN, K_MARKS, K_LINKS, K_EMIT, K_MATERIALIZE, K_CHAIN, K_SPREAD = range(7)


def popcount(x):
    return bin(x).count("1")


def bits(m):
    """Set-bit positions of a mask, ascending."""
    return [t for t in range(32) if (m >> t) & 1]


# ------------------------------------------------------------------ scan, marks
def exclusive_prefix(tot):
    """off[0 .. T] of T counts: off[t] = sum(tot[:t]); off[T] the total."""
    off, run = [], 0
    for v in tot:
        off.append(run)
        run += int(v)
    return off + [run]


def exclusive_prefix_np(tot):
    out = np.zeros(len(tot) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(tot, dtype=np.uint64), out=out[1:])
    return out


def marks(tot, stride, nmark, extra, guard):
    """sh_mark[0 .. 16] after a scan of `tot` with ScanMarks{stride, nmark, extra}."""
    T = len(tot)
    off = exclusive_prefix(tot)
    m = [guard] * 17
    if stride:
        for k in range(nmark):
            if k * stride <= T:
                m[k] = off[k * stride]
    if extra is not None and extra <= T:
        m[nmark] = off[extra]
    return m


# --------------------------------------------------------------------- link emit
def tile_counts(masks):
    return [sum(popcount(int(m)) for m in masks[t:t + TILE]) for t in range(0, len(masks), TILE)]


def chunk_offsets(ttot):
    """coff[0 .. C] of k_chunk_scan: the exclusive prefix over chunks of 64 tiles."""
    return exclusive_prefix([sum(ttot[c:c + CSUM_TILES]) for c in range(0, len(ttot), CSUM_TILES)])


def outdeg_hist(masks):
    h = [0] * OUTDEG_BINS
    for m in masks:
        h[min(popcount(int(m)), OUTDEG_BINS - 1)] += 1
    return h


def new_entries(masks):
    """(parent, position) of every new state, in emit order."""
    return [(i, t) for i, m in enumerate(masks) for t in bits(int(m))]


def link_emit(masks, base, level_gidx, next_gidx, cap, chunk_base):
    """-> (link {o: word}, parent {index: word}, ord {index: byte}, defer_flags, outdeg)."""
    link, parent, ord_ = {}, {}, {}
    flags = 0
    for e, (i, t) in enumerate(new_entries(masks)):
        o = chunk_base + e
        if o >= cap:
            flags |= DF_CAPACITY
            continue
        link[o] = ((base + i) << 8 | t) & M64
        parent[next_gidx + o] = level_gidx + base + i
        ord_[next_gidx + o] = t
    return link, parent, ord_, flags, outdeg_hist(masks)


def new_entries_np(masks):
    """new_entries as two arrays (parent, position)."""
    m = np.ascontiguousarray(masks, dtype="<u4")
    b = np.unpackbits(m.view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    i, t = np.nonzero(b)
    return i.astype(np.uint64), t.astype(np.uint64)


def link_emit_np(masks, base, level_gidx, next_gidx, cap, chunk_base):
    """-> (o, link words, parent words, ord bytes) of the entries below cap (the
    trace entries sit at next_gidx + o), defer_flags, outdeg."""
    i, t = new_entries_np(masks)
    o = np.uint64(chunk_base) + np.arange(len(i), dtype=np.uint64)
    keep = o < np.uint64(min(cap, M64))
    pidx = np.uint64(base) + i
    flags = 0 if bool(keep.all()) else DF_CAPACITY
    cnt = np.minimum(np.unpackbits(np.ascontiguousarray(masks, dtype="<u4").view(np.uint8).reshape(-1, 4),
                                   axis=1).sum(axis=1), OUTDEG_BINS - 1)
    deg = [int(x) for x in np.bincount(cnt, minlength=OUTDEG_BINS)]
    return (o[keep], ((pidx << np.uint64(8)) | t)[keep], (np.uint64(level_gidx) + pidx)[keep], t[keep], flags, deg)


# ------------------------------------------------------------- emit, materialise
class SpecLevel:
    """The parents of a level (canonical tuples) through kubecheck.Spec: per
    parent its successors in TLC order as (action index, tuple)."""

    def __init__(self, spec, tuples):
        from kubecheck._lib import ACTIONS
        self.spec = spec
        self.tuples = np.ascontiguousarray(tuples, dtype=np.uint64)
        self.n = len(self.tuples)
        act = {a: k for k, a in enumerate(ACTIONS)}
        self.nact = len(ACTIONS)
        self.succ = []
        for t in self.tuples:
            s, fail = spec.successors(t)
            assert fail is None, "a parent raises an Assert failure"
            self.succ.append([(act[a], x.copy()) for a, x in s])
        self._packed = None
        self._info = {}

    def packed(self):
        if self._packed is None:
            self._packed = np.concatenate([self.spec.pack(t) for t in self.tuples])
        return self._packed

    def full_masks(self):
        return [(1 << len(s)) - 1 for s in self.succ]

    def info(self, i, t):
        """(packed words, violates an invariant, successor count) of successor t of parent i."""
        if (i, t) not in self._info:
            x = self.succ[i][t][1]
            s, fail = self.spec.successors(x)
            assert fail is None, "a new state raises an Assert failure"
            self._info[i, t] = (self.spec.pack(x), self.spec.check_invariants(x) is not None, len(s))
        return self._info[i, t]


def first_discoverer_masks(level, seen, new=None):
    """newmask words of a level under the rule the engine's default claim
    settles to: a state belongs to its first discoverer in (parent, position)
    order, and states in `seen` (a set of keys: earlier levels and this one)
    are not new.  `seen` grows by the level's new states.  With `new` (the
    keys of the next level) only those states count, and `seen` may start
    empty."""
    masks = []
    for succ in level.succ:
        m = 0
        for t, (_, x) in enumerate(succ):
            k = x.tobytes()
            if k not in seen and (new is None or k in new):
                seen.add(k)
                m |= 1 << t
        masks.append(m)
    return masks


def emit(level, masks, base=0, next_base=0, chunk_base=0, level_gidx=0, next_gidx=0, keep_trace=True):
    """The materialising emit -> dict(next {index: packed words}, parent, ord,
    err_key, act_dist, outdeg, next_cand)."""
    r = dict(next={}, parent={}, ord={}, err_key=M64, act_dist=[0] * level.nact, outdeg=outdeg_hist(masks), next_cand=0)
    for e, (i, t) in enumerate(new_entries(masks)):
        o = chunk_base + e
        words, violates, nsucc = level.info(i, t)
        r["next"][o - next_base] = words
        if keep_trace:
            r["parent"][next_gidx + o] = level_gidx + base + i
            r["ord"][next_gidx + o] = t
        if violates:
            r["err_key"] = min(r["err_key"], (base + i) << 16 | t << 8 | E_INVARIANT)
        r["act_dist"][level.succ[i][t][0]] += 1
        r["next_cand"] += nsucc
    return r


def materialize(prev, links):
    """The rebuild of a deferred frontier from (parent index in the previous
    frontier, position) pairs -> dict(out [packed words per state], defer_flags,
    defer_inv_n, act_dist, next_cand)."""
    r = dict(out=[], defer_flags=0, defer_inv_n=0, act_dist=[0] * prev.nact, next_cand=0)
    first = None
    for i, (pp, t) in enumerate(links):
        words, violates, nsucc = prev.info(pp, t)
        r["out"].append(words)
        if violates and first is None:
            first = i
        r["act_dist"][prev.succ[pp][t][0]] += 1
        r["next_cand"] += nsucc
    if first is not None:
        r["defer_flags"] = DF_INVARIANT
        r["defer_inv_n"] = ~first & M64
    return r


def links_of(link_words):
    return [(int(w) >> 8, int(w) & 0xff) for w in link_words]


# ------------------------------------------------------------------ parent chain
def parent_chain(parent, ord_, g, cap):
    """-> (len, chain words); len 0: longer than cap (the words written so far stay)."""
    out = []
    while True:
        if len(out) >= cap:
            return 0, out
        out.append((g << 8 | ord_[g]) & M64)
        if parent[g] == M64:
            return len(out), out
        g = parent[g]


# ------------------------------------------------------------------------ spread
def spread_tile(b, G, S):
    if S == 0 or S >= G:
        return b
    x, k = b % S, b // S
    return x * (G // S) + min(x, G % S) + k


# ----------------------------------------------------------------------- harness
def selftest(kind, par, a=None, b=None, out=None, res=None, cfg=None):
    """One kc_emit_selftest call (include/kubecheck.h); out and res are uint64
    arrays, changed in place.  Returns the C return code."""
    import ctypes as C

    import kubecheck

    def arr(x):
        return None if x is None else np.ascontiguousarray(x, dtype=np.uint64)

    def ptr(x):
        return None if x is None else x.ctypes.data_as(C.POINTER(C.c_uint64))

    def ln(x):
        return 0 if x is None else len(x)

    par, a, b = arr([int(p) & M64 for p in par]), arr(a), arr(b)
    for x in (out, res):
        assert x is None or (x.dtype == np.uint64 and x.flags.c_contiguous)
    c = (cfg or kubecheck.ModelConfig()).to_c()
    return kubecheck.load().kc_emit_selftest(kind, C.byref(c), ptr(par), ln(par), ptr(a), ln(a), ptr(b), ln(b),
                                             ptr(out), ln(out), ptr(res), ln(res))
