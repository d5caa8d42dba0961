"""The five kernels of bgzf_kernels.hip at their seams, judged by the plain rule of tests/bgzf_rule.py (zlib, a bit-by-bit parse, plain
Huffman and package-merge -- nothing of bgzf_format.hpp) as well as by the host emulation.  Every case goes through the raw launcher
v2p_bgzf_launch on caller-owned device memory and, for each of two workspace fills (0x00: a store that is missing shows; 0xFF: a
shared word that is not zeroed shows), asserts

    out_begin == the rule's (block list + the member sizes walked by BSIZE) == the host emulation's,
    the bytes == the host emulation's, and every device member passes check_member,
    the 4 KiB either side of d_out, every byte of d_out behind out_begin[n_ranges], and the 4 KiB either side of the workspace keep
    their fill.

tests/test_bgzf_rule.py shows on the CPU that the generator's blocks reach every class of R.GEN_CLASSES."""
import ctypes

import numpy as np
import pytest

import bgzf_rule as R

pytestmark = pytest.mark.gpu
SEED = 1
GUARD = 4096
FILLS = (0x00, 0xFF)
OUT_FILL = 0xA5
CU_COUNT_ATTRIBUTE = 63                                                     # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def peek(ptr, n):
    from hip_util import hip
    out = np.empty(n, dtype=np.uint8)
    assert hip().hipDeviceSynchronize() == 0
    assert hip().hipMemcpy(out.ctypes.data, ptr, n, 2) == 0
    return out


class Case:
    """data cut into ranges, the host emulation's answer (computed once), and the members already checked"""
    checked = {}

    def __init__(self, parts):
        from vcf2prot_amd import bgzf
        self.data, self.rb = R.ranges_of(parts)
        self.n_ranges = len(parts)
        self.blocks = R.blocks_of(self.rb)
        self.want, self.want_ob = bgzf.compress_host(self.data, self.rb)
        self.sizes = R.split_members(self.want)
        assert self.want_ob.tolist() == R.out_begin_of(self.rb, self.sizes)  # (the host emulation against the rule, before any launch)

    def run(self, lead=0, ws_fill=0, shift=0, capacity=None):
        """one launch; returns (rc, out_begin, the whole output allocation, its payload offset)"""
        from hip_util import DevBuf, hip
        from vcf2prot_amd import _native as N
        from vcf2prot_amd import bgzf
        lib = N.hip_lib()
        d_in = DevBuf.of(np.frombuffer(b"\xEE" * lead + self.data, dtype=np.uint8))
        d_rb = DevBuf.of(self.rb + np.uint64(lead))
        ws_bytes = lib.v2p_bgzf_workspace_bytes(len(self.data) + lead, self.n_ranges)
        ws = DevBuf(ws_bytes, pad=GUARD, fill=ws_fill)
        assert ws.ptr % 256 == 0
        cap = bgzf.bound(len(self.data), self.n_ranges) if capacity is None else capacity
        out = DevBuf(cap + 8, pad=GUARD, fill=OUT_FILL)
        assert out.ptr % 4 == 0
        d_ob = DevBuf(8 * (self.n_ranges + 1), fill=OUT_FILL)
        try:
            rc = lib.v2p_bgzf_launch(None, d_in.ptr, d_rb.ptr, self.n_ranges, ws.ptr, out.ptr + shift, cap, d_ob.ptr)
            assert hip().hipDeviceSynchronize() == 0
            ob = d_ob.download().view(np.uint64)
            whole = peek(out.base, cap + 8 + 2 * GUARD)
            for where, ptr in (("before", ws.base), ("behind", ws.ptr + ws_bytes)):
                assert (peek(ptr, GUARD) == ws_fill).all(), f"the 4 KiB {where} the workspace changed"
            self.address = d_in.ptr + lead
        finally:
            for b in (d_in, d_rb, ws, out, d_ob):
                b.free()
        return rc, ob, whole, GUARD + shift

    def check(self, **kw):
        rc, ob, whole, at = self.run(**kw)
        assert rc == 0, (rc, kw)
        total = int(ob[-1])
        assert total == len(self.want), (total, len(self.want), kw)
        z = whole[at:at + total].tobytes()
        assert (whole[:at] == OUT_FILL).all() and (whole[at + total:] == OUT_FILL).all(), ("bytes outside the members changed", kw)
        sizes = R.split_members(z)
        assert ob.tolist() == R.out_begin_of(self.rb, sizes), ("out_begin is not the rule's", kw)
        assert ob.tolist() == self.want_ob.tolist(), kw
        first = next((i for i in range(total) if z[i] != self.want[i]), None) if z != self.want else None
        assert first is None, (f"byte {first} differs from the host emulation", kw)
        p = 0
        for (src, n, _), size in zip(self.blocks, sizes):
            key = (z[p:p + size], self.data[src:src + n])
            if key not in Case.checked:
                Case.checked[key] = R.check_member(*key)
                assert Case.checked[key].ours and Case.checked[key].kind in ("stored", "dynamic")
            p += size
        return z

    def members_of(self, ranges):
        """[(member, block)] of one-block ranges, from the host emulation's bytes (which check() found equal to the device's)"""
        return [(self.want[int(self.want_ob[r]):int(self.want_ob[r + 1])], self.data[int(self.rb[r]):int(self.rb[r + 1])]) for r in ranges]


@pytest.fixture(scope="module")
def blocks(built):
    """the generator's blocks with their kinds, decided from the host emulation's members by the rule: {name: (block, kind)}"""
    from vcf2prot_amd import bgzf
    out = {}
    for name, block in R.gen_blocks(SEED):
        rec = R.check_member(bgzf.compress_host(block, [0, len(block)])[0], block)
        out[name] = (block, R.kind_of(block, rec))
    return out


def cu_count():
    """the compute units the compress kernel sizes its grid by.  The attribute's number is the installed header's; should the enum
    ever shift, another attribute would hardly give one of the four counts an MI355X or a partition of it has (8 XCDs of 32 CUs)"""
    from hip_util import hip
    n = ctypes.c_int(0)
    assert hip().hipDeviceGetAttribute(ctypes.byref(n), CU_COUNT_ATTRIBUTE, 0) == 0
    assert n.value in (32, 64, 128, 256), n.value
    return n.value


def test_mixed_blocks_through_one_workgroup(built, gpu_ctx, blocks):
    """5 x the compress kernel's grid (2 x CUs) one-block ranges, so every workgroup's loop runs five times over one CompressLds, and
    block i (workgroup i mod grid) is of kind (round + workgroup) mod 5: each workgroup takes a 3-byte, a stored, a one-symbol, a
    length-limited and an all-256 block in turn.  Blocks are 1 .. 2 300 bytes, except the length-limited ones -- a tree deeper than 15
    needs at least F(18) = 2 584 symbols, the generator's have 10 247 to 21 870 bytes -- and five of 65 279 or 65 280.  The kernel asks the
    runtime for the CU count as cu_count() does."""
    grid = 2 * cu_count()
    order = ("tiny", "stored", "one_symbol", "limited", "all_256")
    pools = {k: sorted((name for name, (b, kind) in blocks.items() if kind == k and len(b) <= (22000 if k == "limited" else 2300)),
                       key=lambda name: len(blocks[name][0]))[:8] for k in order}
    assert all(len(pools[k]) >= 3 for k in order), {k: len(v) for k, v in pools.items()}
    names = []
    for i in range(5 * grid):
        pool = pools[order[(i // grid + i % grid) % 5]]
        names.append(pool[(i // 5) % len(pool)])
    for i, name in ((3, "random_65280"), (grid + 1, "size_65280"), (2 * grid - 1, "size_65279"), (3 * grid + 7, "random_65280"),
                    (4 * grid, "size_65280"), (5 * grid - 1, "fib_scaled_24")):
        names[i] = name
    assert len(names) >= 4 * grid
    for w in range(grid):
        assert len({blocks[n][1] for n in names[w::grid]}) >= 3, (w, names[w::grid])
    case = Case([blocks[n][0] for n in names])
    assert len(case.blocks) == 5 * grid
    for fill in FILLS:
        case.check(ws_fill=fill)


def _seam_ranges(n_ranges, blocks):
    """tiny ranges with empty ones first, last, alone, in runs of 2 and 40 and across range index 1 023 / 1 024; sixty two-block ranges
    early on, so that the block index runs ahead of the range index; a two-block range on block indices 1 023 / 1 024 and a
    three-block range on 2 046 .. 2 048.  Returns (parts, the block indices of the multi-block ranges placed at the seams)."""
    rng = np.random.default_rng(n_ranges)
    tiny = [b for b, _ in blocks.values() if len(b) <= 40] + [blocks["size_254"][0][:k] for k in (5, 9, 17, 33)]
    two, three = blocks["size_65280"][0] + b"ACDEFGH", blocks["size_65279"][0] + blocks["size_65280"][0] + b"KL"
    empty = {0, n_ranges - 1, 100, 200, 201} | set(range(300, 340)) | set(range(1020, 1027))
    parts, n_blocks, seams = [], 0, []
    for r in range(n_ranges):
        if r in empty:
            part = b""
        elif n_blocks == 1023 and r < n_ranges - 1:
            part = two
            seams.append(n_blocks)
        elif n_blocks == 2046 and r < n_ranges - 1:
            part = three
            seams.append(n_blocks)
        elif 1 <= r <= 60:
            part = two
        else:
            part = tiny[int(rng.integers(len(tiny)))]
        parts.append(part)
        n_blocks += -(-len(part) // R.BLOCK)
    return parts, seams


@pytest.mark.parametrize("n_ranges", [1023, 1024, 1025, 2049, 3000])
def test_plan_and_sizes_seams(built, gpu_ctx, blocks, n_ranges):
    """the two scans of 1 024 entries per pass with a carry: range counts either side of one, two and nearly three passes; empty ranges
    where out_begin comes from "the next block, or the total"; ranges whose blocks lie either side of a pass of the sizes scan"""
    parts, seams = _seam_ranges(n_ranges, blocks)
    assert len(parts) == n_ranges and parts[0] == parts[-1] == b"" and seams[:1] == [1023]
    assert n_ranges < 2049 or seams == [1023, 2046]
    case = Case(parts)
    assert n_ranges < 1025 or (parts[1023] == parts[1024] == b"" and case.want_ob[1020] == case.want_ob[min(1027, n_ranges)])
    for fill in FILLS:
        case.check(ws_fill=fill)


def test_every_range_empty(built, gpu_ctx):
    """no block at all: out_begin is zero throughout, nothing is written, with and without an input pointer"""
    from vcf2prot_amd import _native as N
    from hip_util import DevBuf, hip
    for n_ranges in (1, 1025):
        case = Case([b""] * n_ranges)
        assert case.blocks == [] and case.want == b""
        for fill in FILLS:
            case.check(ws_fill=fill)
        d_rb = DevBuf.of(np.full(n_ranges + 1, 77, dtype=np.uint64))
        ws = DevBuf(N.hip_lib().v2p_bgzf_workspace_bytes(0, n_ranges), pad=GUARD, fill=0xFF)
        d_ob = DevBuf(8 * (n_ranges + 1), fill=OUT_FILL)
        try:
            assert N.hip_lib().v2p_bgzf_launch(None, None, d_rb.ptr, n_ranges, ws.ptr, None, 0, d_ob.ptr) == 0
            assert hip().hipDeviceSynchronize() == 0
            assert not d_ob.download().any()
        finally:
            for b in (d_rb, ws, d_ob):
                b.free()


def test_lane_seams_at_every_input_alignment(built, gpu_ctx, blocks):
    """each lane owns 255 bytes and lane 255 adds the end-of-block code: blocks of 1 .. 3, 254 .. 257, 509 .. 511, 65 024 .. 65 026
    (255 x 255 +- 1: the last size at which lane 255 owns the end-of-block code alone), 65 279 and 65 280 bytes, and two-symbol blocks
    of every size in 250 .. 260 (about one bit a byte: lanes 0, 1 and 255 share a word), each starting at every address mod 16.  So
    does the two-symbol sweep of every size from 1 across the stored-to-coded transition: the device decides use_stored from its own
    scan of the data bits, and the sizes where the coded bytes meet n + 5 are where it could decide otherwise.  The ranges between
    them only move the next one to that alignment."""
    from vcf2prot_amd import bgzf
    sweep = [b for b, _ in R.two_symbol_sweep(5, lambda block: bgzf.compress_host(block, [0, len(block)])[0])]
    assert [len(b) for b in sweep] == list(range(1, len(sweep) + 1)) and len(sweep) > 25
    named = [blocks[f"size_{n}"][0] for n in R.SIZES] + [blocks[f"two_symbols_n{n}"][0] for n in range(250, 261)] + sweep
    for lead in range(16):
        parts, at, seam = [], lead, []
        for block in named:
            if (at - lead) % 16:
                parts.append(bytes([65 + lead]) * (16 - (at - lead) % 16))
                at += len(parts[-1])
            seam.append(len(parts))
            parts.append(block)
            at += len(parts[-1])
        case = Case(parts)
        for fill in FILLS:
            case.check(lead=lead, ws_fill=fill)
            assert all((case.address + int(case.rb[r])) % 16 == lead for r in seam), lead
            kinds = [Case.checked[(m, b)].kind for m, b in case.members_of(seam[-len(sweep):])]
            assert kinds[0] == "stored" and kinds[-20:] == ["dynamic"] * 20 and kinds[-21] == "stored", kinds


def test_compaction_into_unaligned_and_exact_outputs(built, gpu_ctx, blocks):
    """d_out at 1, 2 and 3 bytes from a 4-byte boundary; out_capacity == the total: every byte is there and none behind it;
    out_capacity == the total - 1: the launcher returns OK, out_begin[n_ranges] still holds the total, d_out is untouched"""
    parts = [blocks[n][0] for n in ("size_254", "size_3", "size_255", "random_40", "one_symbol_77_40", "size_1", "size_257", "size_2",
                                    "two_symbols_254_255", "random_700", "size_65026", "runs_0", "flat_5x1")]
    case = Case(parts)
    assert {s % 4 for s in case.sizes} == {0, 1, 2, 3} and {int(x) % 4 for x in case.want_ob[:-1]} == {0, 1, 2, 3}
    total = len(case.want)
    for shift in (0, 1, 2, 3):
        for fill in FILLS:
            case.check(ws_fill=fill, shift=shift)
            case.check(ws_fill=fill, shift=shift, capacity=total)
            rc, ob, whole, _ = case.run(ws_fill=fill, shift=shift, capacity=total - 1)
            assert rc == 0 and ob.tolist() == case.want_ob.tolist()
            assert (whole == OUT_FILL).all(), "an output one byte too small was written to"


def test_argument_checks_return_before_any_launch(built, gpu_ctx, blocks):
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.hip_lib()
    case = Case([blocks["size_254"][0]])
    d_in, d_rb = DevBuf.of(np.frombuffer(case.data, dtype=np.uint8)), DevBuf.of(case.rb)
    ws = DevBuf(lib.v2p_bgzf_workspace_bytes(len(case.data), 1), pad=GUARD, fill=0x5A)
    out, d_ob = DevBuf(1024, pad=GUARD, fill=OUT_FILL), DevBuf(16, fill=OUT_FILL)
    try:
        good = [None, d_in.ptr, d_rb.ptr, 1, ws.ptr, out.ptr, 1024, d_ob.ptr]
        for what, at, value in (("null d_range_begin", 2, None), ("null workspace", 4, None), ("workspace not aligned to 256", 4, ws.ptr + 128),
                                ("workspace not aligned to 256", 4, ws.ptr + 1), ("null d_out_begin", 7, None), ("n_ranges = 2^32", 3, 1 << 32),
                                ("null d_out with a capacity", 5, None)):
            args = list(good)
            args[at] = value
            assert lib.v2p_bgzf_launch(*args) == N.V2P_ERR_INVALID_ARG, what
        assert hip().hipDeviceSynchronize() == 0
        assert (peek(ws.base, ws.nbytes + 2 * GUARD) == 0x5A).all() and (peek(out.base, 1024 + 2 * GUARD) == OUT_FILL).all()
        assert (d_ob.download() == OUT_FILL).all()
        assert lib.v2p_bgzf_launch(*good) == 0
        assert out.download()[:len(case.want)].tobytes() == case.want
    finally:
        for b in (d_in, d_rb, ws, out, d_ob):
            b.free()
