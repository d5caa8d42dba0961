"""stitchw_kernel's ROW-COUNT BODIES (csrc/stitch_wave.hip: wave_rows<R>): a chunk runs the body of 10, 9 or 8 rows by the 1 KiB rows its
result ends in -- block space, so a host-packed chunk's ragged head counts; chunks of fewer than 8 rows run the 8-row body.  Hand-built
images (tests/stitch_rule.py, tests/stitch_cases.py) through v2p_stitch_launch_opts of the product library on guarded buffers
(hip_util.stitch_launch), judged by the plain rule: the status word, EVERY byte of the arena, the guards.  Every builder asserts first, from
positions alone (stitch_rule.Layout), that its chunks end where the case says.

  the seams of the dispatch   test_single_chunk_ends_at_a_seam       one chunk ending at 16 B, 7 rows, 8 192 / 9 216 (-16, +0, +1, +16), 10 240 (-16, +0):
                                                                     host form with head 0, host form with head 15 (head + total crosses, not total), rows form
  the last row of a body      test_last_row_of_each_body             per body: a record ending on the row line, the chunk ending on it, a cut last block (whole and
                                                                     ragged), a replaced residue in the last block and in the first block of the last row, an
                                                                     immediate ending the chunk, 64 descriptors; nt x sc1
  neighbours in other bodies  test_neighbouring_chunks_of_every_pair chunks of 1, 7, 8, 9, 10 rows, all 25 ordered pairs adjacent: host form back to back (shared
                                                                     blocks), rows form (head skip, tail clip across the short chunks), rows form in phases of
                                                                     eight chunks (read-ahead on the trailing workgroups); "nt" and "sc1 nt" stores
  the staged instance         test_c3_slice_staged_then_resident     a C3 slice through build_and_execute (rows staged per phase), two re-executes from resident
                                                                     rows, arena scribbled in between, digests and bytes against the C oracle; the image holds chunks
                                                                     of at most 7, of 8, 9 and 10 rows.  (Only a batch has staging buffers: the raw launcher cannot
                                                                     reach the staged instance, and v2p_batch_set_packed takes no rows-form chunk table.)
  refusals                    test_refusals_are_what_they_were       641 blocks: STATUS_RES_OOB; a descriptor past its source in a 9-row chunk: STATUS_SRC_OOB at it;
                                                                     neither chunk writes a byte, their neighbours of 8, 9 and 10 rows are written"""
import numpy as np
import pytest

import stitch_cases as C
import stitch_rule as R
from stitch_rule import F, Image, Layout, P, Y, imm, snv3

pytestmark = pytest.mark.gpu

ROW = 1024


def rows_of(L):
    """the 1 KiB rows a chunk's result ends in, in block space: what the kernel's dispatch looks at"""
    return (L.ptotal + ROW - 1) // ROW if L.total else 0


def fill(total, n=None):
    """`total` bytes as n descriptors, proteome and payload runs taking turns, neighbours of unequal length (record lines off the block lines)"""
    assert total >= 1
    n = min(max(n or 1, -(-total // 1500)), total)                  # (no run longer than the payload tape allows)
    base = total // n
    assert base <= 3000
    lens = [base] * n
    for k in range(0, n - 1, 2):
        if base > 7:
            lens[k] += 7
            lens[k + 1] -= 7
    lens[-1] += total - sum(lens)
    return [P((131 * i) % 4000, ln) if i % 2 == 0 else Y((53 * i) % 1000, ln) for i, ln in enumerate(lens)]


def check(im, what, **opts):
    """launch the image, print the figures, compare status, every byte of the arena, the guards"""
    from hip_util import stitch_launch
    want, want_status = R.run_rule(im)
    want = np.frombuffer(want, np.uint8)
    desc, chunks = im.arrays()
    got, status, guards = stitch_launch(desc, chunks, im.src0, im.src1, im.out_len, opts)
    diff = np.nonzero(got != want)[0]
    print(f"{what} {opts}: status {status:#x} (rule {want_status:#x}), {diff.size} of {im.out_len} bytes differ"
          + (f", first at {int(diff[0])}: got {int(got[diff[0]]):#x}, rule {int(want[diff[0]]):#x}" if diff.size else "") + f", guards {'intact' if guards else 'CHANGED'}")
    assert guards, f"{what}: a guard region changed"
    assert status == want_status, f"{what}: status {status:#x}, the rule says {want_status:#x}"
    assert diff.size == 0, f"{what}: {diff.size} bytes differ, the first at {int(diff[0])}"


# ---- the seams of the dispatch ----
SEAMS = [16, 7 * ROW, 8 * ROW - 16, 8 * ROW, 8 * ROW + 1, 8 * ROW + 16, 9 * ROW - 16, 9 * ROW, 9 * ROW + 1, 9 * ROW + 16, 10 * ROW - 16, 10 * ROW]


@pytest.mark.parametrize("form", ["host", "head", "rows"])
@pytest.mark.parametrize("size", SEAMS)
def test_single_chunk_ends_at_a_seam(built, size, form):
    im = Image()
    head = 15 if form == "head" else 0
    if form == "rows":
        im.add(fill(size), dst=0, flag=C.ROWS)
    else:
        im.add(fill(size - head), dst=32 + head)
    L = Layout(im, 0)
    assert L.head == head and L.ptotal == size and rows_of(L) == -(-size // ROW) and im.out_len == im.cursor
    if form == "head":                                               # (8 192 + 1, 9 216 + 1: the head carries the chunk across the row line, its total alone ends a row earlier)
        assert -(-L.total // ROW) == rows_of(L) - (1 if 0 < size % ROW <= head else 0)
    check(im, f"{form} {size}", nontemporal=1, store_sc1=0)


# ---- the last present row of each body ----
def last_row_image(rows):
    base = (rows - 1) * ROW
    im, at = Image(), [0]

    def add(descs, head=0):
        c = im.add(descs, dst=at[0] + head)
        at[0] += 16384
        L = Layout(im, c)
        assert rows_of(L) == rows and L.head == head, (rows, rows_of(L), L.ptotal)
        return L

    L = add(fill(base) + [Y(9, 500)])                                # a record ends exactly on the line of the last row
    assert any(e == base for _, e, _, _ in L.recs)
    L = add(fill(rows * ROW))                                        # ... and on the row's end: the chunk fills its body
    assert L.ptotal == rows * ROW
    L = add(fill(base + 400 - 9) + [Y(77, 9)])                       # a cut block as the chunk's last block, whole
    assert L.ptotal % 16 == 0 and L.recs[-1][0] == L.ptotal - 9
    L = add(fill(base + 400 - 9) + [Y(77, 4)])                       # ... and ragged
    assert L.ptotal % 16 == 11 and L.recs[-1][0] // 16 == L.nblk - 1
    L = add(fill(base + 200) + [snv3(500, 100, 3, ord("r"))])        # a replaced residue in the last block
    assert L.recs[-1][3] // 16 == L.nblk - 1 and L.ptotal == base + 304
    L = add(fill(base - 20) + [snv3(600, 25, 200, ord("s"))])        # ... and in the first block of the last row
    assert L.recs[-1][3] == base + 5
    L = add(fill(base - 20 - 7) + [snv3(600, 25, 200, ord("t"))], head=7)      # ... the head carrying it there
    assert L.recs[-1][3] == base + 5
    L = add(fill(base + 100) + [imm(b"end")])                        # an immediate record ends the chunk, ragged
    assert L.recs[-1][2] == "imm" and L.ptotal % 16 == 7
    L = add(fill(base + 109) + [imm(b"end")])                        # ... and on a block line
    assert L.recs[-1][2] == "imm" and L.ptotal % 16 == 0
    L = add([P(3 * i, 100) if i % 2 else Y(5 * i, 100) for i in range(63)] + [P(40, base + 500 - 6300)])      # 64 descriptors
    assert L.n == 64 and L.ptotal == base + 500
    return im


@pytest.mark.parametrize("sc1", [0, 1])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("rows", [8, 9, 10])
def test_last_row_of_each_body(built, rows, nt, sc1):
    check(last_row_image(rows), f"last row of body {rows}", nontemporal=nt, store_sc1=sc1)


# ---- neighbouring chunks in different bodies ----
ROW_COUNTS = (1, 7, 8, 9, 10)


def every_pair_sequence(vals):
    """a sequence in which every ordered pair of vals (equal ones too) is adjacent once: an Euler circuit of the complete digraph with loops"""
    out_edges = {a: list(vals) for a in vals}
    stack, seq = [vals[0]], []
    while stack:
        a = stack[-1]
        if out_edges[a]:
            stack.append(out_edges[a].pop())
        else:
            seq.append(stack.pop())
    seq.reverse()
    assert {(a, b) for a, b in zip(seq, seq[1:])} == {(a, b) for a in vals for b in vals} and len(seq) == len(vals) ** 2 + 1
    return seq


def neighbours_host():
    """host form, back to back: neighbours share 16-byte blocks, every chunk's head is where the one before it ended"""
    rng = np.random.default_rng(7)
    seq = every_pair_sequence(ROW_COUNTS)
    im = Image()
    im.add(fill(21), dst=0)                                          # (so that the first chunk of the sequence has a ragged head too)
    for k, r in enumerate(seq):
        head = im.cursor & 15
        lo, hi = max((r - 1) * ROW + 1 - head, 1), r * ROW - head
        total = hi if k % 4 == 0 else int(rng.integers(lo, hi + 1))       # (every fourth chunk ends on its body's last byte)
        d = fill(total, n=int(rng.integers(1, 40)))
        if k % 3 == 0:                                               # a replaced residue and an immediate at the chunk's end
            d = fill(total - 40 - 3, n=int(rng.integers(1, 40))) + [snv3(700 + k, 30, 9, ord("a") + k % 26), imm(b"xyz")]
        c = im.add(d)
        assert rows_of(Layout(im, c)) == r and Layout(im, c).head == head
    assert [rows_of(Layout(im, c)) for c in range(1, len(im.chunks))] == seq
    return im


def neighbours_rows():
    """rows form: one descriptor stream cut on the rows of the sequence -- a descriptor across a cut is head skip in one chunk, tail clip in the other"""
    rng = np.random.default_rng(8)
    seq = every_pair_sequence(ROW_COUNTS)
    need = sum(seq) * ROW
    d = []
    while sum(map(R.desc_len, d)) < need + 400:
        k = (0, 0, 0, 1, 1, 1, 2, 3, 4, 4)[int(rng.integers(0, 10))]
        d.append([P(int(rng.integers(0, 6000)), int(rng.integers(100, 500))), Y(int(rng.integers(0, 3000)), int(rng.integers(100, 500))), F(int(rng.integers(60, 200))),
                  imm(b"lit"), snv3(int(rng.integers(0, 6000)), int(rng.integers(0, 300)), int(rng.integers(0, 300)), ord("s"))][k])
    im = Image()
    cuts = [0] + [int(x) for x in np.cumsum(seq) * ROW]
    got = C.cut_rows(im, d, cuts)
    assert [rows_of(Layout(im, c)) for c in range(len(im.chunks))] == seq and max(g[2] for g in got) <= 64
    short = [g for g, r in zip(got, seq) if r < 10]
    assert sum(g[0] > 0 for g in short) > 10 and sum(g[1] > 0 for g in short) > 10          # head skips and tail clips across the short chunks
    return im


_images = {}


def neighbours(form):
    if form not in _images:
        _images[form] = neighbours_host() if form == "host" else neighbours_rows()
    return _images[form]


@pytest.mark.parametrize("sc1", [0, 1])
@pytest.mark.parametrize("form", ["host", "rows", "rows in phases"])
def test_neighbouring_chunks_of_every_pair(built, form, sc1):
    im = neighbours(form.split()[0])
    opts = dict(nontemporal=1, store_sc1=sc1)
    if form == "rows in phases":
        n = len(im.chunks)
        per_chunk = 16 + 8 * len(im.desc) / n                        # the launcher's measure of a chunk (stitch_kernels.hip: phase_plan)
        opts.update(phase_min_chunks=1, phase_bytes=int(8.5 * per_chunk))
        assert max(8, int(opts["phase_bytes"] / per_chunk) & ~7) == 8 and n > 3 * 8 and n % 8 != 0
    check(im, f"neighbours, {form}", **opts)


# ---- the staged instance: a device-built C3 slice, staged per phase at its first execute, from resident rows afterwards ----
def test_c3_slice_staged_then_resident(built, gpu_ctx, coracle):
    from resident_rows_util import SMALL, check as check_haps, cohort, reexecute, upload
    h0, n = 20, 12
    gpu_ctx.upload_proteome(cohort().proteome())
    rs = upload(gpu_ctx, h0, n)
    b = gpu_ctx.batch()
    try:
        gpu_ctx.set_launch_opts(**SMALL)
        b.build_and_execute(rs, 6, 0)
        b.sync()
        check_haps(b, coracle, h0, n, "first execute", bytes_too=True)
        reexecute(b, coracle, h0, n, "re-execute 1", bytes_too=True)
        reexecute(b, coracle, h0, n, "re-execute 2")
        _, chunks, _ = b.download_image()
        assert ((chunks[:, 1] >> np.uint64(59)) & np.uint64(3) == 3).all()           # wave chunks of a rows image, every one
        dst = np.sort((chunks[:, 1] & np.uint64(R.DST_MASK)) & ~np.uint64(1023)).astype(np.int64)
        size = np.diff(np.concatenate([dst, [b.counts()["out_bytes"]]]))
        rows = -(-size // ROW)
        hist = {r: int((rows == r).sum()) for r in range(1, 11)}
        print(f"rows per chunk of the slice: {hist}")
        assert rows.max() == 10 and hist[10] > 100 and hist[9] > 100 and hist[8] > 30 and sum(hist[r] for r in range(1, 8)) > 10
    finally:
        gpu_ctx.set_launch_opts()
        b.scribble()
        b.close()
        rs.close()


# ---- refusals ----
@pytest.mark.parametrize("nt", [0, 1])
def test_refusals_are_what_they_were(built, nt):
    im = Image()
    a = im.add(fill(8 * ROW - 100), dst=0)
    big = C._limit_chunk(im, 16384, 0, 0, extra=1)                   # 641 blocks
    b9 = im.add(fill(9 * ROW - 50), dst=2 * 16384 + 3)
    d = fill(8 * ROW + 300)
    d[3] = P(R.SRC0_LEN - 16, R.desc_len(d[3]))                      # a descriptor that reads past the proteome, in a 9-row chunk
    bad = im.add(d, dst=3 * 16384)
    c10 = im.add(fill(10 * ROW), dst=4 * 16384)
    assert Layout(im, big).nblk == 641 and rows_of(Layout(im, bad)) == 9 and R.desc_len(d[3]) > 16
    assert [rows_of(Layout(im, c)) for c in (a, b9, c10)] == [8, 9, 10]
    want, status = R.run_rule(im)
    assert status == ((im.chunks[big][0] << 8) | R.STATUS_RES_OOB) and status < (((im.chunks[bad][0] + 3) << 8) | R.STATUS_SRC_OOB)
    assert set(want[16384:16384 + 10241]) == {R.SENTINEL} and set(want[3 * 16384:3 * 16384 + 8 * ROW + 300]) == {R.SENTINEL}      # neither writes a byte
    check(im, "refusals", nontemporal=nt, store_sc1=0)
    im2 = Image()                                                    # the bad descriptor alone: its own status word
    im2.add(fill(8 * ROW - 100), dst=0)
    bad2 = im2.add(d, dst=16384)
    assert R.run_rule(im2)[1] == (((im2.chunks[bad2][0] + 3) << 8) | R.STATUS_SRC_OOB)
    check(im2, "bad descriptor in a 9-row chunk", nontemporal=nt, store_sc1=0)
