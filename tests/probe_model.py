"""A plain host model of the seen-set tables (helper module, no tests here).

Written from the comments of csrc/fpset_dev.h, engine_kernels.h (lds_claim)
and DESIGN §3, with Python integers: every table is open addressing with
linear probing from a home slot, slots fill in probe order and are never
cleared, so a fingerprint sits before the first empty slot of its run.

  kind      slot                    home
  "fpset"   u64 fp                  mulhi(fp * G, nslots)
  "wide"    {fp, ~claim} (16 B)     mulhi(fp * G, nslots)
  "compact" u64 fp                  2 * mulhi(fp * G, nslots / 2)   (even)
  "batch"   {fp, ~min key}          mix(fp) & (nslots - 1)
  "lds"     {fp, min key (u32)}     low 32 bits of fp: & 2047 for 2048 entries,
                                    mulhi32(fp, nslots) otherwise

claim = level << 44 | key; a slot stores ~claim, so the largest stored word
is the smallest claim; a claim word of 0 is "pending, current level".

kc_probe_selftest (tests/test_gpu_probe.py) runs the device primitives on the
same inputs; in its sequential mode results and table images must be equal.
"""
import random

G = 0x9e3779b97f4a7c15
M64 = (1 << 64) - 1
GINV = pow(G, -1, 1 << 64)
CL_OLD, CL_LOST, CL_CUR, CL_NEW, CL_FULL = 0, 1, 2, 3, 4
KEY_BITS = 44
LDS_NT, LDS_NT_SH = 2048, 1792
LDS_EMPTY_KEY = 0xFFFFFFFF
CLAIM_BATCH = 2          # k_claim's pipelined group (KC_CLAIM_BATCH)

# kc_probe_selftest kinds (include/kubecheck.h)
(PK_FPSET_INSERT, PK_FPSET_CONTAINS, PK_CLAIM, PK_CLAIM_STORE, PK_CLAIM_GET, PK_INSERT_FROM, PK_PAIR, PK_PAIR_GROUP,
 PK_PAIR_STALE, PK_BATCH, PK_LDS, PK_LDS_SH, PK_REHASH_CLAIMSET, PK_REHASH_FPSLOTS, PK_REHASH_FPSET) = range(15)

WORDS = {"fpset": 1, "compact": 1, "wide": 2, "batch": 2, "lds": 2}


def mulhi(x, n):
    return (x * n) >> 64


def home(fp, nslots, kind):
    if kind in ("fpset", "wide"):
        return mulhi((fp * G) & M64, nslots)
    if kind == "compact":
        return 2 * mulhi((fp * G) & M64, nslots // 2)
    if kind == "batch":
        h = fp ^ (fp >> 29)
        h = (h * 0xbf58476d1ce4e5b9) & M64
        return (h >> 21) & (nslots - 1)
    if kind == "lds":
        lo = fp & 0xFFFFFFFF
        return lo & (LDS_NT - 1) if nslots == LDS_NT else (lo * nslots) >> 32
    raise ValueError(kind)


def make_claim(level, key):
    return (level << KEY_BITS) | key


def nclaim(level, key):
    return ~make_claim(level, key) & M64


def craft(slot, nslots, kind, count, rng, top=None):
    """`count` distinct fingerprints (0 < fp < 2^63) whose home is `slot`:
    draw in the slot's range of the remixed space and multiply by G^-1."""
    out = []
    seen = set()
    if kind == "lds":
        while len(out) < count:
            if nslots == LDS_NT:
                lo = (rng.getrandbits(21) << 11) | slot
            else:
                a, b = -(-(slot << 32) // nslots), -(-((slot + 1) << 32) // nslots)
                lo = rng.randrange(a, b)
            fp = (rng.getrandbits(31) << 32) | lo
            if 0 < fp < 1 << 63 and fp not in seen and home(fp, nslots, kind) == slot:
                seen.add(fp)
                out.append(fp)
        return out
    nb, b = (nslots // 2, slot // 2) if kind == "compact" else (nslots, slot)
    lo, hi = -(-(b << 64) // nb), -(-((b + 1) << 64) // nb)
    while len(out) < count:
        fp = (rng.randrange(lo, hi) * GINV) & M64
        if 0 < fp < 1 << 63 and fp not in seen:
            assert home(fp, nslots, kind) == slot
            seen.add(fp)
            out.append(fp)
    return out


class Table:
    """One table; `w` is its image as kc_probe_selftest copies it out."""

    def __init__(self, nslots, kind, image=None):
        self.n, self.kind, self.wps = nslots, kind, WORDS[kind]
        if image is not None:
            self.w = [int(x) for x in image]
            assert len(self.w) == nslots * self.wps
        else:
            self.w = [0] * (nslots * self.wps)
            if kind == "lds":
                self.w[1::2] = [LDS_EMPTY_KEY] * nslots

    def fp_at(self, i):
        return self.w[i * self.wps]

    def run(self, fp, start=None):
        """Slots in probe order: every slot once, from the home, wrapping."""
        s = home(fp, self.n, self.kind) if start is None else start % self.n
        for k in range(self.n):
            yield (s + k) % self.n

    def locate(self, fp, start=None):
        """(slot, True) where fp is stored, (slot, False) for the first empty
        slot of its run when it is not, (None, False) when the table is full."""
        for i in self.run(fp, start):
            f = self.fp_at(i)
            if f == fp:
                return i, True
            if f == 0:
                return i, False
        return None, False

    def occupied(self):
        return {i for i in range(self.n) if self.fp_at(i)}

    def fps(self):
        return sorted(self.fp_at(i) for i in range(self.n) if self.fp_at(i))

    # -- first-claim inserts (fpset, compact, 16-B insert_from): the fp word only
    def insert(self, fp, start=None):
        i, found = self.locate(fp, start)
        if i is None:
            return CL_FULL
        if found:
            return CL_OLD
        self.w[i * self.wps] = fp
        return CL_NEW

    def fpset_insert(self, fp):
        return {CL_NEW: 1, CL_OLD: 0, CL_FULL: -1}[self.insert(fp)]

    def contains(self, fp):
        return 1 if self.locate(fp)[1] else 0

    # -- compact table: the pair {home, home + 1} is read together.  Present in
    # the pair as read: old.  Else the run goes on from the first slot of the
    # pair that read empty (whatever it holds by now), or past the pair.
    def pair_start(self, fp, e=None):
        h = home(fp, self.n, "compact")
        e = (self.w[h], self.w[h + 1]) if e is None else e
        if fp in e:
            return None
        return h if e[0] == 0 else h + 1 if e[1] == 0 else h + 2

    def pair_insert(self, fp, e=None):
        s = self.pair_start(fp, e)
        return CL_OLD if s is None else self.insert(fp, s)

    def pair_group(self, fps):
        """k_claim's order for a group: all first loads, then every CAS into
        its pair's first empty slot as loaded, then each claim carries on."""
        starts = [self.pair_start(fp) for fp in fps]
        cas = []
        for fp, s in zip(fps, starts):
            h = home(fp, self.n, "compact")
            if s is None or s == h + 2:
                cas.append(None)
                continue
            cas.append(self.w[s])
            if self.w[s] == 0:
                self.w[s] = fp
        res = []
        for fp, s, c in zip(fps, starts, cas):
            if s is None:
                res.append(CL_OLD)
            elif c is None:
                res.append(self.insert(fp, s))
            elif c == 0:
                res.append(CL_NEW)
            elif c == fp:
                res.append(CL_OLD)
            else:
                res.append(self.insert(fp, s + 1))
        return res

    # -- 16-B slots
    def _settle(self, i, nc, level, store):
        seen = self.w[2 * i + 1]
        if seen != 0 and ((~seen & M64) >> KEY_BITS) < level:
            return CL_OLD                    # an earlier level's entry: no write
        if seen != 0 and seen >= nc:
            return CL_LOST                   # a smaller claim is stored
        if store:
            self.w[2 * i + 1] = nc
        return CL_CUR

    def claim(self, fp, key, level, store=True):
        """claimset_claim (store=True: the claim is folded in at once) and the
        claim launch of the STORE-claim protocol (store=False: only the
        inserter writes its claim; a candidate writes nothing)."""
        nc = nclaim(level, key)
        i, found = self.locate(fp)
        if i is None:
            return CL_FULL
        if found:
            return self._settle(i, nc, level, store)
        self.w[2 * i], self.w[2 * i + 1] = fp, nc
        return CL_NEW

    def store_claim(self, fp, key, level):
        i, found = self.locate(fp)
        if found:
            self.w[2 * i + 1] = max(self.w[2 * i + 1], nclaim(level, key))

    def get(self, fp):
        i, found = self.locate(fp)
        return self.w[2 * i + 1] if found else 0

    def store_protocol(self, fps, keys, level):
        """The three launches; returns (codes, holds-the-claim flags)."""
        codes = [self.claim(fp, k, level, store=False) for fp, k in zip(fps, keys)]
        for fp, k, c in zip(fps, keys, codes):
            if c == CL_CUR:
                self.store_claim(fp, k, level)
        return codes, [int(self.get(fp) == nclaim(level, k)) for fp, k in zip(fps, keys)]

    # -- batch table and LDS tile table: the minimum key per fingerprint
    def batch(self, fps, keys):
        for fp, k in zip(fps, keys):
            i, found = self.locate(fp)
            assert i is not None
            self.w[2 * i] = fp
            self.w[2 * i + 1] = max(self.w[2 * i + 1], ~k & M64)
        return [int(self.get(fp) == (~k & M64)) for fp, k in zip(fps, keys)]

    def lds_claim(self, fp, lk):
        i, found = self.locate(fp)
        if i is None:
            return -1
        self.w[2 * i] = fp
        self.w[2 * i + 1] = min(self.w[2 * i + 1], lk)
        return i

    # -- what holds for a table in any insertion order
    def check_runs(self):
        """Every stored fingerprint lies on its run before the first empty slot."""
        for i in range(self.n):
            fp = self.fp_at(i)
            if fp:
                assert self.locate(fp) == (i, True), (i, hex(fp))


def rehash(old, new_nslots):
    """The model of a rehash: every entry of `old` in a new table (claim
    words travel with their fingerprints)."""
    nw = Table(new_nslots, old.kind)
    for i in range(old.n):
        fp = old.fp_at(i)
        if fp:
            j, found = nw.locate(fp)
            assert j is not None and not found
            nw.w[j * nw.wps: (j + 1) * nw.wps] = old.w[i * old.wps: (i + 1) * old.wps]
    return nw


def rng(seed):
    return random.Random(seed)
