"""A plain host model of the seen-set's cold tier (helper module, no tests
here), written from csrc/coldset.h and coldset.hip with Python integers and
sorted numpy arrays.

Keys: cold_key / cold_unkey, the splitmix64 finaliser and its inverse.

ColdModel follows kc::ColdSet in what it holds and in what it counts, not in
how it searches: a key is found iff it is in a run.
  add_run   push the run; while the last two runs are both in host RAM and
            (a.n * 2 <= b.n * 3 or there are more than 12 runs) merge them;
            while host_bytes is set and exceeded, the oldest host run becomes
            a file run of ceil(n / window_keys) windows; then the newest runs
            get HBM copies of their keys (cache_keys) as the budget allows.
  probe     runs newest first; a query whose found byte is already 1 is left
            alone.  A run with a filter that is not read by the merge-probe
            counts a filter test per query not yet found when the run is
            reached.  A file run without an HBM copy is read by windows:
            window w holds the queries in [first key of w, first key of w + 1)
            (the first window starts at 0), is read iff it holds one, and a
            window read costs 8 bytes per key of it.
  build_meta  dbits by the code's loop; filter bits per key min(bloom_bits,
            bytes left * 8 / n), no filter below 4; nblocks = max(1, n * bits
            / 512): meta_bytes exactly.
The Bloom hash is not modelled: of filter_passed the model gives the lower
bound `filtered_hits` (hits found in runs with a filter) only.

kc_coldset_* (tests/test_gpu_coldset.py) drives the real ColdSet with the
same calls; stats() has the order of kc_coldset_stats.
"""
import random

import numpy as np

M64 = (1 << 64) - 1
M1, M2 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
I1, I2 = pow(M1, -1, 1 << 64), pow(M2, -1, 1 << 64)
ENOMEM, EINVAL = 12, 22
MSEG = 2048                 # keys per merge-probe segment
MERGE_RANGE = 65536         # merged keys per thread range

STATS = ("runs", "runs_disk", "keys", "host_bytes", "disk_bytes", "meta_bytes", "peak_meta_bytes", "merges",
         "merged_keys", "disk_written", "disk_read", "windows_skipped", "cached_runs", "cached_keys", "cache_bytes",
         "cache_uploaded", "filter_tests", "filter_passed", "merge_probes")
# what the model gives exactly (everything but filter_passed)
EXACT = tuple(s for s in STATS if s != "filter_passed")


def cold_key(fp):
    z = fp & M64
    z = ((z ^ (z >> 30)) * M1) & M64
    z = ((z ^ (z >> 27)) * M2) & M64
    return z ^ (z >> 31)


def _unxorshift(y, s):
    x = y
    for _ in range(s, 64, s):
        x = y ^ (x >> s)
    return x


def cold_unkey(k):
    z = (_unxorshift(k & M64, 31) * I2) & M64
    z = (_unxorshift(z, 27) * I1) & M64
    return _unxorshift(z, 30)


def dir_bits(n):
    dbits = 1
    while (1 << (dbits + 1)) * 16 <= n and dbits < 40:
        dbits += 1
    return dbits


def dir_bytes(n):
    return ((1 << dir_bits(n)) + 1) * 8


def merge_ranges(n_merged, merge_threads):
    """Key ranges (threads) the host merge of n_merged keys is cut into."""
    return max(1, min(merge_threads, n_merged // MERGE_RANGE + 1))


def u64(keys):
    return np.array(sorted(int(k) for k in keys), dtype=np.uint64)


class Run:
    def __init__(self, keys):
        self.keys = keys                 # sorted np.uint64
        self.n = len(keys)
        self.host = True                 # in pinned host RAM (else a file)
        self.cached = False              # HBM copy of the keys
        self.has_dir = False
        self.bits = 0                    # filter bits per key (0 = no filter)
        self.nblocks = 0
        self.meta_bytes = 0
        self.wkeys = self.nw = 0

    @property
    def bytes(self):
        return self.n * 8

    def contains(self, q):
        """np.bool_ per query."""
        i = np.searchsorted(self.keys, q)
        return self.keys[np.minimum(i, self.n - 1)] == q


class ColdModel:
    def __init__(self, meta_hbm_bytes=0, host_bytes=0, spill_dir=False, window_keys=1 << 23, bloom_bits=10,
                 cache_keys=True, merge_div=0, merge_threads=16):
        self.budget, self.host_budget, self.spill_dir = meta_hbm_bytes, host_bytes, bool(spill_dir)
        self.window_keys = max(64, window_keys) & ~7
        self.bloom_bits, self.cache_keys, self.merge_div = bloom_bits, bool(cache_keys), merge_div
        self.merge_threads = max(1, merge_threads)
        self.runs = []                   # oldest first
        self.failed = False
        self.error = ""
        self.merge_range_log = []        # ranges of every merge so far
        self.clear()

    def clear(self):
        self.runs = []
        self.failed = False
        self.keys = self.host_used = self.disk_used = self.meta_used = self.cache_used = 0
        self.peak_meta = 0
        self.merges = self.merged_keys = self.disk_written = self.disk_read = self.windows_skipped = 0
        self.cache_uploaded = self.filter_tests = self.merge_probes = 0
        self.filtered_hits = 0           # lower bound of filter_passed

    # ---- HBM budget: directories and filters come before key copies
    def _uncache(self, r):
        if r.cached:
            r.cached = False
            self.cache_used -= r.bytes

    def _make_room(self, nbytes):
        if not self.budget:
            return
        for r in self.runs:
            if self.meta_used + self.cache_used + nbytes <= self.budget:
                return
            self._uncache(r)

    def _build_meta(self, r):
        db = dir_bytes(r.n)
        self._make_room(db + self.bloom_bits * r.n // 8 + 64)
        if self.budget and self.meta_used + db > self.budget:
            self.error = "HBM budget for cold-run directories exhausted"
            return -ENOMEM
        r.has_dir = True
        r.meta_bytes = db
        self.meta_used += db
        bits = self.bloom_bits
        if self.budget:
            left = self.budget - self.meta_used - self.cache_used
            assert left >= 0
            bits = min(bits, left * 8 // r.n)
        if bits >= 4:
            r.bits = bits
            r.nblocks = max(1, r.n * bits // 512)
            r.meta_bytes += r.nblocks * 64
            self.meta_used += r.nblocks * 64
        self.peak_meta = max(self.peak_meta, self.meta_used + self.cache_used)
        return 0

    def _free(self, r):
        self._uncache(r)
        self.meta_used -= r.meta_bytes
        if r.host:
            self.host_used -= r.bytes
        else:
            self.disk_used -= r.bytes
        self.keys -= r.n

    def _recache(self):
        if not self.cache_keys:
            return
        for r in reversed(self.runs):
            if r.cached:
                continue
            if self.budget and self.meta_used + self.cache_used + r.bytes > self.budget:
                break
            r.cached = True
            self.cache_used += r.bytes
            self.cache_uploaded += r.bytes
            if not r.host:               # a file run streams back through the staging windows
                self.disk_read += r.bytes
        self.peak_meta = max(self.peak_meta, self.meta_used + self.cache_used)

    # ---- the calls
    def add_run(self, keys):
        """0, or -ENOMEM (self.error says which); keys: strictly ascending."""
        assert not self.failed
        r = Run(np.asarray(keys, dtype=np.uint64))
        assert r.n > 0 and (r.n == 1 or bool((r.keys[1:] > r.keys[:-1]).all()))
        self.host_used += r.bytes
        self.keys += r.n
        rc = self._build_meta(r)
        self.runs.append(r)
        if rc:
            self.failed = True
            return rc
        while len(self.runs) >= 2:
            a, b = self.runs[-2], self.runs[-1]
            if not (a.host and b.host):
                break
            if not (a.n * 2 <= b.n * 3 or len(self.runs) > 12):
                break
            c = Run(np.sort(np.concatenate([a.keys, b.keys]), kind="stable"))
            self.host_used += c.bytes
            self.merges += 1
            self.merged_keys += c.n
            self.merge_range_log.append(merge_ranges(c.n, self.merge_threads))
            self._free(self.runs.pop())
            self._free(self.runs.pop())
            self.keys += c.n
            rc = self._build_meta(c)
            self.runs.append(c)
            if rc:
                self.failed = True
                return rc
        while self.host_budget and self.host_used > self.host_budget:
            hosts = [x for x in self.runs if x.host]
            if not hosts:
                break
            if not self.spill_dir:
                self.error = "no spill directory"
                self.failed = True
                return -ENOMEM
            x = hosts[0]
            x.host = False
            x.wkeys = self.window_keys
            x.nw = (x.n + x.wkeys - 1) // x.wkeys
            self.host_used -= x.bytes
            self.disk_used += x.bytes
            self.disk_written += x.bytes
        self._recache()
        return 0

    def probe(self, q, found=None, hits=0):
        """(found bytes, hits) after probing the ascending queries q."""
        assert not self.failed
        q = np.asarray(q, dtype=np.uint64)
        m = len(q)
        assert m > 0 and bool((q[1:] >= q[:-1]).all())
        found = np.zeros(m, dtype=np.uint8) if found is None else np.array(found, dtype=np.uint8)
        for r in reversed(self.runs):
            todo = found == 0
            here = todo & r.contains(q)
            if not r.cached and r.host and self.merge_div > 0 and m >= r.n // self.merge_div:
                self.merge_probes += 1
            elif r.cached or r.host:
                if r.bits:
                    self.filter_tests += int(todo.sum())
                    self.filtered_hits += int(here.sum())
            else:
                # window w: queries in [bound[w], bound[w + 1]), bound[0] = 0, past the last = every query left
                bound = [0] + [int(r.keys[w * r.wkeys]) for w in range(1, r.nw)]
                qa = [int(np.searchsorted(q, np.uint64(b), side="left")) for b in bound] + [m]
                for w in range(r.nw):
                    if qa[w + 1] <= qa[w]:
                        self.windows_skipped += 1
                        continue
                    self.disk_read += (min(r.n, (w + 1) * r.wkeys) - w * r.wkeys) * 8
                    if r.bits:
                        self.filter_tests += int(todo[qa[w]:qa[w + 1]].sum())
                if r.bits:
                    self.filtered_hits += int(here.sum())
            found[here] = 1
            hits += int(here.sum())
        return found, hits

    def all_keys(self):
        """The sorted multiset of every key added (reads the file runs)."""
        assert not self.failed
        for r in self.runs:
            if not r.host:
                self.disk_read += r.bytes
        if not self.runs:
            return np.zeros(0, dtype=np.uint64)
        return np.sort(np.concatenate([r.keys for r in self.runs]), kind="stable")

    def stats(self):
        """The exact fields of kc_coldset_stats by name (no filter_passed)."""
        s = {
            "runs": len(self.runs), "runs_disk": sum(not r.host for r in self.runs), "keys": self.keys,
            "host_bytes": self.host_used, "disk_bytes": self.disk_used, "meta_bytes": self.meta_used,
            "peak_meta_bytes": self.peak_meta, "merges": self.merges, "merged_keys": self.merged_keys,
            "disk_written": self.disk_written, "disk_read": self.disk_read, "windows_skipped": self.windows_skipped,
            "cached_runs": sum(r.cached for r in self.runs), "cached_keys": sum(r.n for r in self.runs if r.cached),
            "cache_bytes": self.cache_used, "cache_uploaded": self.cache_uploaded, "filter_tests": self.filter_tests,
            "merge_probes": self.merge_probes,
        }
        assert tuple(s) == EXACT
        return s


# ---- key sets of the shapes the kernels could go wrong on (sorted np.uint64)
def rng(seed):
    return random.Random(seed)


def shape_keys(shape, n, r):
    if shape == "uniform":
        s = set()
        while len(s) < n:
            s.add(r.getrandbits(64))
    elif shape == "low":                  # the lowest n integers, key 0 included
        s = range(n)
    elif shape == "high":                 # the highest n, 2^64 - 1 included
        s = range(M64 - n + 1, M64 + 1)
    elif shape == "mid":                  # n consecutive keys around 2^63
        s = range((1 << 63) - n // 2, (1 << 63) - n // 2 + n)
    elif shape == "cluster":              # one top-16-bit prefix: the whole run in one directory bucket
        top = r.getrandbits(16) << 48
        s = set()
        while len(s) < n:
            s.add(top | r.getrandbits(48))
    elif shape == "mixed":                # uniform and cluster interleaved
        top = r.getrandbits(16) << 48
        s = set()
        while len(s) < n:
            s.add(top | r.getrandbits(48) if len(s) % 2 else r.getrandbits(64))
    else:
        raise ValueError(shape)
    return u64(s)


def standard_queries(keys, r, extra=300):
    """Every present key, its neighbours, the ends and the middle of the key
    space, and `extra` random words: sorted, distinct."""
    s = set()
    for k in (int(x) for x in keys):
        s.update((k, (k + 1) & M64, (k - 1) & M64))
    s.update((0, M64, 1 << 63, (1 << 63) - 1))
    s.update(r.getrandbits(64) for _ in range(extra))
    return u64(s)


def key_inputs(oracle):
    """The ends and the middle of the word range, random words, and Model_1
    fingerprints (the words the engine keys)."""
    import kubecheck
    r = rng(1)
    words = [0, 1, 1 << 63, M64] + [r.getrandbits(64) for _ in range(3000)]
    spec = kubecheck.Spec(kubecheck.ModelConfig())
    for level in (1, 9, 40):
        words += [spec.fingerprint(t) for t in oracle.level_tuples(oracle.config(), level)[:300]]
    return np.array(words, dtype=np.uint64)
