"""Helpers of the distinct-record tests: hand-built arenas between guard regions for v2p_unique_add_records, and the comparison of a set
with the rule (tests/unique_rule.py)."""
import numpy as np

import unique_rule as U

GUARD = 0xA5
GUARD_BYTES = 256


def layout(records, align=None, gap=b""):
    """(key, residues) records laid out back to back (with `gap` between them) -> (arena bytes, begins).  align[i] (optional): filler is put
    in front of record i until its first byte sits at that offset modulo 16."""
    arena, begins = bytearray(), []
    for i, (_, res) in enumerate(records):
        if i:
            arena += gap
        if align is not None and align[i] is not None:
            while len(arena) % 16 != align[i]:
                arena.append(0x7E)
        begins.append(len(arena))
        arena += res
    return bytes(arena), begins


class Arena:
    """records on the device: the arena `misalign` bytes behind a 16-byte line between two guard regions, the three record arrays (and
    forced digests) beside it"""

    def __init__(self, records, begins, arena: bytes, misalign=0, digests=None):
        from hip_util import DevBuf, hip
        self.records, self.n = list(records), len(records)
        self.arena_len, self.at = len(arena), GUARD_BYTES + misalign
        host = np.full(GUARD_BYTES + misalign + len(arena) + GUARD_BYTES, GUARD, np.uint8)
        host[self.at:self.at + len(arena)] = np.frombuffer(arena, np.uint8)
        self.image = host.copy()
        self.buf = DevBuf.of(host)
        assert self.buf.ptr % 16 == 0
        self.d_begin = DevBuf.of(np.asarray(list(begins) + [0], np.uint64))
        self.d_len = DevBuf.of(np.asarray([len(r) for _, r in records] + [0], np.uint32))
        self.d_key = DevBuf.of(np.asarray([k for key, _ in records for k in key] + [0, 0], np.uint64))
        self.d_dig = DevBuf.of(np.asarray(digests, np.uint64).reshape(-1)) if digests is not None else None
        self._hip = hip

    def add(self, uset):
        """(class_of, info); the arena and its guards must be as they were"""
        try:
            return uset.add_records(self.buf.ptr + self.at, self.arena_len, self.d_begin.ptr, self.d_len.ptr, self.d_key.ptr, self.n,
                                    self.d_dig.ptr if self.d_dig else 0)
        finally:
            assert np.array_equal(self.buf.download(), self.image), "the arena or its guards changed"

    def scribble(self, byte):
        assert self._hip().hipMemset(self.buf.base, byte, self.buf.nbytes + 2 * self.buf.pad) == 0
        self.image[:] = byte

    def free(self):
        for b in (self.buf, self.d_begin, self.d_len, self.d_key, self.d_dig):
            if b:
                b.free()


def arena_of(records, misalign=0, align=None, gap=b"", digests=None):
    arena, begins = layout(records, align, gap)
    return Arena(records, begins, arena, misalign, digests)


def check_set(uset, records, class_of_parts):
    """the set against the rule on every record added so far (records: (key, residues), key = two integers); class_of_parts: what the adds returned"""
    want_of, want = U.unique_classes(records)
    got_of = np.concatenate([np.asarray(p, np.uint32) for p in class_of_parts]) if class_of_parts else np.zeros(0, np.uint32)
    assert got_of.tolist() == want_of
    cls, counts = uset.classes(), uset.counts()
    assert counts["n_classes"] == len(want) and counts["n_records"] == len(records)
    assert counts["store_bytes"] == sum(len(c["residues"]) + 1 for c in want)
    assert cls["key"].tolist() == [list(c["key"]) for c in want]
    assert cls["len"].tolist() == [len(c["residues"]) for c in want]
    assert cls["count"].tolist() == [c["count"] for c in want]
    assert cls["first_record"].tolist() == [c["first_record"] for c in want]
    order = list(range(len(want)))
    assert uset.emit(order) == U.emit_text(want, order)
    return want
