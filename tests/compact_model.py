"""The rule of include/mfa_compact.h in numpy over raw bytes (a plain module like tree_model.py: no test, no fixture): the caches of the six
configurations tests/test_compact_gpu.py runs -- contiguous, token-major and paged, filled with bytes that identify (sequence, head, slot,
K or V) -- the model of the launch with its drop rules and newLengths, the wrong kernels (MUTANTS) the case list must tell from it, and the
case list itself, CASES, which tests/test_compact_sensitivity.py (CPU) and tests/test_compact_gpu.py (GPU) share."""
import collections
import functools

import numpy as np

B, HKV, CAPACITY = 3, 2, 256
ELEMENT_BYTES = {"e4m3": 1, "bf16": 2, "f16": 2}

Config = collections.namedtuple("Config", "D element layout page shuffled")
CONFIGS = (
    Config(64, "e4m3", "contiguous", 0, False),
    Config(64, "bf16", "token-major", 0, False),
    Config(128, "f16", "paged", 16, True),
    Config(128, "e4m3", "paged", 16, True),
    Config(256, "bf16", "contiguous", 0, False),
    Config(256, "e4m3", "paged", 64, False),
)


class Geometry(collections.namedtuple("Geometry", "row_bytes ld hs outer column page table pages")):
    """byte strides of one cache buffer (K and V alike): a row of head h at key `pos` of sequence b starts at
    slot(b, pos)[0] x outer + slot(b, pos)[1] x ld + h x hs.  page 0: contiguous, `outer` the batch stride; else `outer` the page stride and
    `table` int32 [B][stride] the block table the launch is given (its width is blockTableStride)"""

    def slot(self, b, pos):
        """(page or sequence, key inside it), or None for a row the append launch's rules drop"""
        if pos < 0:
            return None
        if self.page:
            index = pos // self.page
            if index >= self.table.shape[1] or self.table[b, index] < 0:
                return None
            return int(self.table[b, index]), pos % self.page
        return (b, pos) if pos < self.column else None

    def at(self, slot, h):
        return slot[0] * self.outer + slot[1] * self.ld + h * self.hs


def _words(b, h, pos, which, count):
    """`count` uint32 words that identify (sequence, head, slot, K or V) and their own place in the row"""
    w = np.arange(count, dtype=np.uint64)
    x = (b + 1) * 0x9E3779B1 + (h + 1) * 0x85EBCA6B + (pos + 1) * 0xC2B2AE35 + (which + 1) * 0x27D4EB2F + (w + 1) * 0x165667B1
    x ^= x >> np.uint64(15)
    return (x * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def build(config, edit=None):
    """-> (K, V flat uint8 arrays, Geometry), built once per (config, edit) and shared: read them, do not write them.  Every slot of every sequence holds its identifying bytes, whatever the lengths; pages no
    table names hold 0xA5.  edit: ("short", keys) -- the table handed over is only keys // page entries wide; ("negative", ((b, key), ...))
    -- the entries of those keys' pages are negative.  Contiguous caches take no edit."""
    rb = config.D * ELEMENT_BYTES[config.element]
    if config.layout == "contiguous":
        geo = Geometry(rb, rb, CAPACITY * rb, HKV * CAPACITY * rb, CAPACITY, 0, None, 0)
        size = B * geo.outer
    elif config.layout == "token-major":
        geo = Geometry(rb, HKV * rb, rb, CAPACITY * HKV * rb, CAPACITY, 0, None, 0)
        size = B * geo.outer
    else:
        page, pps = config.page, CAPACITY // config.page
        pages = B * pps + 2                                     # two pages nobody names
        order = np.random.default_rng(config.D + page).permutation(pages) if config.shuffled else np.arange(pages)
        table = order[:B * pps].reshape(B, pps).astype(np.int32)
        geo = Geometry(rb, rb, page * rb, HKV * page * rb, CAPACITY, page, table, pages)
        size = pages * geo.outer
    bufs = [np.full(size, 0xA5, dtype=np.uint8) for _ in range(2)]
    for which, buf in enumerate(bufs):
        for b in range(B):
            for h in range(HKV):
                for pos in range(CAPACITY):
                    at = geo.at(geo.slot(b, pos), h)
                    buf[at:at + rb] = _words(b, h, pos, which, rb // 4).view(np.uint8)
    if geo.page and edit:
        table = geo.table.copy()
        if edit[0] == "short":
            table = np.ascontiguousarray(table[:, :edit[1] // geo.page])
        else:
            for b, key in edit[1]:
                table[b, key // geo.page] = -1 - b
        geo = geo._replace(table=table)
    return bufs[0], bufs[1], geo


MUTANTS = (
    "in_place",            # rows copied in place in path order without reading first
    "unclamped_P",         # P = cacheLengths - rows: no clamp at 0, queryLengths ignored
    "scatter",             # accepted[i] taken as the destination
    "batch0_path",         # batch 0's path used for every sequence
    "v_unmoved",           # V left unmoved
    "head0_only",          # only head 0 moved
    "source_page",         # the source's page used for the destination
    "a_not_clamped",       # a not clamped to live
    "clamp_index",         # an out-of-range index clamped instead of dropped
    "newlen_unclamped",    # newLengths = n - qn + count
)


def plan(geo, lens, rows, qlens, counts, max_accepted, b):
    """(n, qn, P, live, a) of sequence b"""
    length = int(lens[b])
    n = length if geo.page else min(length, geo.column)
    qn = rows if qlens is None else min(int(qlens[b]), rows)
    live = min(qn, n)
    return n, qn, max(n - qn, 0), live, min(int(counts[b]), max_accepted, live)


def compact(k, v, geo, lens, rows, qlens, accepted, counts, max_accepted, mutant=None):
    """-> (K, V, newLengths uint32 [B]) after the launch; the inputs are left as they are.  mutant: one of MUTANTS, a wrong kernel"""
    assert mutant is None or mutant in MUTANTS
    out = [k.copy(), v.copy()]
    new = np.zeros(len(lens), dtype=np.uint32)
    rb = geo.row_bytes
    for b in range(len(lens)):
        n, qn, P, live, a = plan(geo, lens, rows, qlens, counts, max_accepted, b)
        if mutant == "unclamped_P":
            P = int(lens[b]) - rows
        if mutant == "a_not_clamped":
            a = min(int(counts[b]), max_accepted)
        new[b] = (n - qn + int(counts[b]) if mutant == "newlen_unclamped" else P + a) % 2 ** 32
        path = accepted[0 if mutant == "batch0_path" else b]
        for which, before in enumerate((k, v)):
            if which == 1 and mutant == "v_unmoved":
                continue
            for h in range(1 if mutant == "head0_only" else HKV):
                for i in range(a):
                    j = int(path[i])
                    if mutant == "clamp_index" and live:
                        j = min(max(j, 0), live - 1)
                    if j < 0 or j >= live:
                        continue
                    src, dst = (P + i, P + j) if mutant == "scatter" else (P + j, P + i)
                    s, d = geo.slot(b, src), geo.slot(b, dst)
                    if s is None or d is None:
                        continue
                    if mutant == "source_page" and geo.page:
                        d = (s[0], d[1])
                    source = out[which] if mutant == "in_place" else before
                    out[which][geo.at(d, h):geo.at(d, h) + rb] = source[geo.at(s, h):geo.at(s, h) + rb]
    return out[0], out[1], new


# ---- the case list: every configuration crossed with every path.  LENS / ROWS: the default batch -- P = 188, 65 and 118, none a multiple of
# a page, and the 12 tree rows of sequences 0 and 2 straddle a page of 16 AND a page of 64 (keys 192 and 128)
LENS, ROWS = (200, 77, 130), 12
Path = collections.namedtuple("Path", "name lens rows qlens accepted counts edit")


def _path(name, accepted, counts, lens=LENS, rows=ROWS, qlens=None, edit=None):
    width = max(len(a) for a in accepted)
    table = np.full((B, width), -1, dtype=np.int32)
    for b, a in enumerate(accepted):
        table[b, :len(a)] = a
    return Path(name, tuple(lens), rows, None if qlens is None else tuple(qlens), table, tuple(counts), edit)


_ALL = list(range(ROWS))
_MIXED = [11, 10, 9, 8, 0, 1, 2]   # from sequence 0's second page into its first, and (i = 4) from its first into its second
PATHS = (
    _path("identity", [_ALL] * 3, (12, 12, 12)),
    _path("the first a nodes", [_ALL] * 3, (3, 5, 1)),
    _path("increasing with gaps", [[0, 2, 5, 9, 11], [0, 3, 4, 10], [1, 6, 7, 8, 11]], (5, 4, 5)),
    _path("reversal of 64 nodes", [list(range(63, -1, -1))] * 3, (64, 64, 64), lens=(200, 77, 64), rows=64),
    _path("rotation by one", [_ALL[1:] + [0], _ALL[3:] + [0, 1, 2], [11] + _ALL[:11]], (12, 12, 12)),
    _path("a repeated index", [[3, 3, 3, 7, 7], [5, 5], [0, 0, 11, 11, 0]], (5, 2, 5)),
    _path("a = 0", [[5, 4, 3], [2, 1, 0], [7, 7, 7]], (0, 0, 0)),
    _path("count above live", [[11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 1, 2, 3]] * 3, (16, 100, 2 ** 31 + 5)),
    _path("indices -1 and live", [[2, -1, 5, 12, 0, -7, 64, 11], [12, 11, -1, 0], [-2 ** 31, 2 ** 31 - 1, 3, 12]], (8, 4, 4)),
    _path("n < qn", [[4, 0, 2, 1, 3, 5], [2, 1, 0, 3], [10, 9, 11, 0]], (6, 4, 4), lens=(5, 3, 11)),
    _path("cacheLengths above column", [[11, 0, 5], [3, 2, 1, 0], [6, 6]], (3, 4, 2), lens=(300, 256, 1000)),
    _path("a length of 0", [[1, 0], [4, 3, 2], [0]], (2, 3, 1), lens=(0, 200, 0)),
    _path("per-sequence queryLengths", [[11, 3, 7], [4, 0, 5, 1], [2, 1]], (3, 4, 2), qlens=(20, 5, 0)),
    _path("sources and destinations straddle a page", [_MIXED, [6, 0, 3], [11, 10, 0, 1, 9]], (7, 3, 5)),
    _path("a table row too short for the destination", [_MIXED, [6, 0, 3], [11, 10, 0, 1, 9]], (7, 3, 5), edit=("short", 192)),
    _path("a negative table entry", [_MIXED, [6, 0, 3], [11, 10, 0, 1, 9]], (7, 3, 5), edit=("negative", ((0, 192), (2, 128)))),
)
CASES = tuple((config, path) for config in CONFIGS for path in PATHS)


def case_id(case):
    config, path = case
    return "d%d-%s-%s%s-%s" % (config.D, config.element, config.layout, config.page or "", path.name.replace(" ", "_"))


def run(case, mutant=None):
    """-> (K, V, Geometry before the launch, (K, V, newLengths) after it) of a case, by the model or a mutant"""
    config, path = case
    k, v, geo = build(config, path.edit)
    return k, v, geo, compact(k, v, geo, path.lens, path.rows, path.qlens, path.accepted, path.counts, path.accepted.shape[1], mutant)
