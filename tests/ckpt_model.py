"""A plain host model of the checkpoint file (helper module, no tests here).

Written from the "Checkpoint" block of include/kubecheck.h alone, with Python
integers and struct: an independent reader and writer of DIR/checkpoint.kc and
the checksum rule, none of it through the library.

  header  64 little-endian u64 words (see WORDS below)
  sections, at the offsets the header names:
    COUNTERS      level_width[nlevels], act_gen[22], act_dist[22], outdeg[16],
                  probes, settles, cand_ovf, narrow_probes
    FRONTIER      n x state_words words
    FPS           distinct words, any order
    TRACE_PARENT  (level_gidx + n) words         (keep_trace only)
    TRACE_ORD     (level_gidx + n) bytes, zero-padded to 8   (keep_trace only)
  checksum = (sum mod 2^64, xor) of the u64 words covered
"""
import os
import struct

M64 = (1 << 64) - 1
MAGIC = int.from_bytes(b"KUBECKPT", "little")
VERSION = 1
HEADER_WORDS = 64
HEADER_BYTES = HEADER_WORDS * 8
SECTIONS = ("COUNTERS", "FRONTIER", "FPS", "TRACE_PARENT", "TRACE_ORD")
NACTIONS = 22
OUTDEG_BINS = 16
COUNTER_TAIL = 2 * NACTIONS + OUTDEG_BINS + 4

# header words 4..24 by name, in file order
MODEL_FIELDS = ("nc", "np", "ns", "can_fail", "can_timeout", "check_deadlock", "variant", "invariants", "symmetry",
                "state_words")
FIELDS = MODEL_FIELDS + ("keep_trace", "claim_mode", "level", "level_gidx", "n", "cand", "cand_total", "init",
                         "distinct", "nlevels", "peak_frontier")
W_FILE_BYTES, W_FIELD0, W_NSECTIONS, W_SECTION0, W_SUM, W_XOR = 3, 4, 25, 26, 62, 63
assert W_FIELD0 + len(FIELDS) == W_NSECTIONS

FILE_NAME = "checkpoint.kc"


def path(d):
    return os.path.join(str(d), FILE_NAME)


def checksum(words):
    s = x = 0
    for w in words:
        s = (s + w) & M64
        x ^= w
    return s, x


def to_words(b):
    assert len(b) % 8 == 0
    return list(struct.unpack("<%dQ" % (len(b) // 8), b))


def to_bytes(words):
    return struct.pack("<%dQ" % len(words), *words)


def pad8(b):
    return b + b"\0" * (-len(b) % 8)


class Checkpoint:
    """The decoded file: `fields` (FIELDS by name) and the sections as word
    lists (TRACE_ORD as the byte string, unpadded)."""

    def __init__(self, fields, level_width, counters, frontier, fps, parent=None, ord_=None):
        self.fields = dict(fields)
        self.level_width = list(level_width)
        self.counters = list(counters)          # the COUNTER_TAIL words after the widths
        self.frontier = list(frontier)
        self.fps = list(fps)
        self.parent = None if parent is None else list(parent)
        self.ord = None if ord_ is None else bytes(ord_)

    def __getattr__(self, k):
        try:
            return self.__dict__["fields"][k]
        except KeyError:
            raise AttributeError(k)

    # the COUNTERS section's named parts
    @property
    def act_gen(self):
        return self.counters[:NACTIONS]

    @property
    def act_dist(self):
        return self.counters[NACTIONS:2 * NACTIONS]

    @property
    def outdeg(self):
        return self.counters[2 * NACTIONS:2 * NACTIONS + OUTDEG_BINS]

    def section_bytes(self):
        out = [to_bytes(self.level_width + self.counters), to_bytes(self.frontier), to_bytes(self.fps)]
        if self.parent is not None:
            out += [to_bytes(self.parent), pad8(self.ord)]
        else:
            out += [b"", b""]
        return out

    def image(self, offsets=None):
        """The file's bytes; `offsets` overrides where the sections go (tests
        of overlapping and out-of-file sections rewrite the header anyway)."""
        secs = self.section_bytes()
        w = [0] * HEADER_WORDS
        w[0], w[1], w[2] = MAGIC, VERSION, HEADER_WORDS
        for k, name in enumerate(FIELDS):
            w[W_FIELD0 + k] = int(self.fields[name])
        w[W_NSECTIONS] = len(SECTIONS)
        body = b""
        for s, b in enumerate(secs):
            if not b:
                continue
            off = HEADER_BYTES + len(body) if offsets is None else offsets[s]
            sm, x = checksum(to_words(b))
            w[W_SECTION0 + 4 * s: W_SECTION0 + 4 * s + 4] = [off, len(b), sm, x]
            body += b
        w[W_FILE_BYTES] = HEADER_BYTES + len(body)
        return seal(w) + body

    def write(self, d):
        with open(path(d), "wb") as f:
            f.write(self.image())


def seal(w):
    """Header words with their checksum (words 62, 63) filled in, as bytes."""
    w = list(w)
    w[W_SUM], w[W_XOR] = checksum(w[:W_SUM])
    return to_bytes(w)


def reseal(image, edit):
    """`image` with its header words changed by edit(words) and the header's
    checksum made right again: what a damaged writer, not a damaged disk, leaves."""
    w = to_words(image[:HEADER_BYTES])
    edit(w)
    return seal(w) + image[HEADER_BYTES:]


def read(d):
    """Parse DIR/checkpoint.kc, checking everything the header promises."""
    with open(path(d), "rb") as f:
        data = f.read()
    return parse(data)


def parse(data):
    assert len(data) >= HEADER_BYTES, "short file"
    w = to_words(data[:HEADER_BYTES])
    assert w[0] == MAGIC and w[1] == VERSION and w[2] == HEADER_WORDS
    assert w[W_FILE_BYTES] == len(data)
    assert (w[W_SUM], w[W_XOR]) == checksum(w[:W_SUM]), "header checksum"
    assert w[W_NSECTIONS] == len(SECTIONS)
    assert all(x == 0 for x in w[W_SECTION0 + 4 * len(SECTIONS):W_SUM])
    f = {name: w[W_FIELD0 + k] for k, name in enumerate(FIELDS)}
    secs = []
    spans = []
    for s in range(len(SECTIONS)):
        off, ln, sm, x = w[W_SECTION0 + 4 * s: W_SECTION0 + 4 * s + 4]
        if ln == 0:
            assert (off, sm, x) == (0, 0, 0)
            secs.append(b"")
            continue
        assert off % 8 == 0 and off >= HEADER_BYTES and off + ln <= len(data), SECTIONS[s]
        b = data[off:off + ln]
        assert checksum(to_words(b)) == (sm, x), SECTIONS[s] + " checksum"
        spans.append((off, off + ln))
        secs.append(b)
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping sections"
    states = f["level_gidx"] + f["n"]
    assert f["distinct"] == states and f["nlevels"] == f["level"]
    assert len(secs[0]) == (f["nlevels"] + COUNTER_TAIL) * 8
    assert len(secs[1]) == f["n"] * f["state_words"] * 8
    assert len(secs[2]) == f["distinct"] * 8
    if f["keep_trace"]:
        assert len(secs[3]) == states * 8 and len(secs[4]) == (states + 7) // 8 * 8
        assert secs[4][states:] == b"\0" * (len(secs[4]) - states)
    else:
        assert not secs[3] and not secs[4]
    cw = to_words(secs[0])
    lw = cw[:f["nlevels"]]
    assert sum(lw) == f["distinct"] and lw[-1] == f["n"]
    return Checkpoint(f, lw, cw[f["nlevels"]:], to_words(secs[1]), to_words(secs[2]),
                      to_words(secs[3]) if f["keep_trace"] else None,
                      secs[4][:states] if f["keep_trace"] else None)


def synthetic(keep_trace=True, seed=7):
    """A small, self-consistent checkpoint: W = 4, three levels of widths
    2, 3, 5, the last the frontier."""
    import random
    r = random.Random(seed)
    lw = [2, 3, 5]
    n, gidx = lw[-1], sum(lw[:-1])
    distinct = gidx + n
    fields = dict(nc=1, np=1, ns=1, can_fail=1, can_timeout=1, check_deadlock=1, variant=0, invariants=3, symmetry=0,
                  state_words=4, keep_trace=int(keep_trace), claim_mode=0, level=3, level_gidx=gidx, n=n, cand=17,
                  cand_total=40, init=2, distinct=distinct, nlevels=3, peak_frontier=3)
    counters = [r.randrange(100) for _ in range(COUNTER_TAIL)]
    frontier = [r.getrandbits(64) for _ in range(n * 4)]
    fps = [r.getrandbits(63) | 1 for _ in range(distinct)]
    parent = [M64, M64] + [r.randrange(0, 2 + k // 2) for k in range(distinct - 2)] if keep_trace else None
    ord_ = bytes(r.randrange(20) for _ in range(distinct)) if keep_trace else None
    return Checkpoint(fields, lw, counters, frontier, fps, parent, ord_)
