"""The named cases of tests/test_rows_cases.py (CPU) and tests/test_gpu_rows_seams.py (GPU): hand-built transcript streams for the
one-pass image builder (csrc/build_rows.hip), each asserting from positions alone -- before anything runs -- that it reaches the seam it
is named after (test helper: numpy only, no import from the project).

The expected bytes are the plain rule of stream_util.random_stream: a transcript's result starts as '.', every Task copies
src[sp : sp + ln] to out[sr : sr + ln] (src: the transcript's reference for code 0, its alt tape for code 1); FASTA wraps the result in its
record header and a line feed; a haplotype is its transcripts back to back.

Geometry of the parse, restated from the kernel: a TILE is K consecutive transcripts; its ITEMS are its Tasks in order, a transcript
without Tasks being one item; a window is 64 items, the first one starts at item 0 and every further one ADV items later; a window emits
its lanes [CTX, 62) -- the first from lane 0, the last to the tile's end."""
import numpy as np

# vcf2prot_amd/csrc/sir_pack.hpp
ROW_BYTES, PIECE_MAX, ROWS_FUSE_LEN, SNV5_MAX_LEN, IMM_MAX_BYTES, ROWS_TILE_SLOTS = 1024, 2047, 1023, 31, 5, 256
CHUNK_TASKS_WAVE, CHUNK_TASKS_DEEP = 64, 1024
# vcf2prot_amd/csrc/rows_image.hpp
ROWS_SEG, ROWS_MAX_WAVE, ROWS_MAX_DENSE = 640, 10, 12
# vcf2prot_amd/csrc/build_rows.h
ROWS_CHUNK_PAD = 96
# vcf2prot_amd/csrc/build_rows.hip (rows_parse_kernel: CTX = 4 for a dense image, else 2; ADV = 62 - CTX; a tile image is parsed as a wave image is)
ROWS_ALT_LDS = 512
CTX = {6: 2, 7: 4, 9: 2}
ADV = {k: 62 - c for k, c in CTX.items()}
# vcf2prot_amd/csrc/dense_pieces.h
TILE_SPAN_MAX, PIECE_BYTES, TILE_SLOTS_MAX = 16368, 16, 2048
# vcf2prot_amd/csrc/sir_pack.hpp
PAD_BYTES_PER_TASK_MAX = 125
# include/vcf2prot_hip.h
ERR_BAD_CODE, ERR_RES_OOB, ERR_SRC_OOB, ERR_NOT_CONTIGUOUS, ERR_UNSUPPORTED = -3, -4, -5, -6, -9

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
DOT = 0x2E

CASES = {}          # name -> (group, builder)


def case(group, name=None):
    def reg(fn):
        CASES[name or fn.__name__] = (group, fn)
        return fn
    return reg


def windows(n_items, kernel):
    """[(R0, e_lo, e_hi, last)] of a tile of n_items"""
    out, R0 = [], 0
    while True:
        last = R0 + 64 >= n_items
        out.append((R0, 0 if R0 == 0 else CTX[kernel], min(n_items - R0, 64) if last else 62, last))
        if last:
            return out
        R0 += ADV[kernel]


def emitted_at(j, n_items, kernel):
    """(window, lane) that emits item j of a tile of n_items"""
    hits = [(w, j - R0) for w, (R0, lo, hi, _) in enumerate(windows(n_items, kernel)) if lo <= j - R0 < hi]
    assert len(hits) == 1, (j, n_items, kernel, hits)
    return hits[0]


class Case:
    """A stream under construction, then the case: arrays for stream_util.Stream, the K to force, the kernels it applies to, the expected bytes."""

    def __init__(self, prot_len=8192, fasta=False, seed=1):
        rng = np.random.default_rng(1000 + seed)
        self.prot = AA[rng.integers(0, 20, size=prot_len)].copy()
        self.fasta = fasta
        self.headers = bytearray(b"\n")
        self.tx, self.hap_tx_begin = [], [0]
        self.K, self.kernels = [1], (6, 7)
        self.two_pass = None           # True / False: what the build info of a wave or dense build must say (None: not claimed)
        self.src64 = False             # run under V2P_ROWS_SRC64
        self.error = None              # (code, task index): build_on_device must refuse with it
        self.refused = {}              # kernel -> error code of a refusal that is not a bad Task (a row with too many descriptors, a tile too long)
        self.onecall_fell_back = None  # True / False: what the one call's build info must say for a wave image (None: not claimed)
        self.cut_emit_pass = None      # True / False: ... whether the emitting pass of a WAVE image's cutter replaced the padded pass
        self.slices = ()               # also built by the one call in this many slices (development library)
        self.pieces = None             # tile images: (pieces of the forced tile 0, slots the statistics give it)
        self.check_image = None        # fn(case, packed, kernel): reach assertions on the HOST image (chunk cuts)
        self.reach = {}                # what the builder established, for the suite-wide coverage assertions

    # ---- building ----
    def open(self, off=0, ref_len=None, header=None):
        t = dict(off=off, ref_len=len(self.prot) - off if ref_len is None else ref_len, tasks=[], alt=bytearray(), cur=0, extra=0, nsp=1, hoff=0, hlen=0, header=b"")
        if header is not None:
            assert self.fasta
            name = (">" + header + "\n").encode()
            t.update(hoff=len(self.headers), hlen=len(name), header=name)
            self.headers += name
        self.tx.append(t)
        return len(self.tx) - 1

    @property
    def t(self):
        return self.tx[-1]

    def n_tasks(self):
        return sum(len(t["tasks"]) for t in self.tx)

    def ref(self, sp, ln, sr=None):
        t = self.t
        sr = t["cur"] if sr is None else sr
        t["tasks"].append((0, sp, ln, sr))
        t["cur"] = sr + ln
        return self.n_tasks() - 1

    def alt(self, data, sr=None):
        t = self.t
        sr = t["cur"] if sr is None else sr
        t["tasks"].append((1, len(t["alt"]), len(data), sr))
        t["alt"] += bytes(data)
        t["cur"] = sr + len(data)
        return self.n_tasks() - 1

    def raw(self, code, sp, ln, sr, advance=True):
        """a Task as given (the offenders of the error cases)"""
        self.t["tasks"].append((code, sp, ln, sr))
        if advance:
            self.t["cur"] = sr + ln
        return self.n_tasks() - 1

    def gap(self, n):
        self.t["cur"] += n

    def tail(self, n):
        self.t["extra"] = n

    def take(self, ln, step=3):
        """a source range of the open transcript that continues nothing before it"""
        t = self.t
        if t["nsp"] + ln + step > t["ref_len"]:
            t["nsp"] = 1
        sp = t["nsp"]
        t["nsp"] += ln + step
        return sp

    def fillers(self, n, ln=17):
        """n reference copies that fuse with nothing: no literal between them, no source continues the one before (17 bytes: a 1 KiB row
        of them holds 61 descriptors, which a wave chunk takes)"""
        return [self.ref(self.take(ln), ln) for _ in range(n)]

    def mixed(self, n, ln=17):
        """n items that fuse with nothing, by turns a reference copy (which the fusion state holds until the next item is known) and an alt
        payload of more than IMM_MAX_BYTES (which it never holds): the held bits of neighbouring lanes differ, so a window that inherits
        them from the wrong lane shows"""
        out = []
        for k in range(n):
            if len(self.t["tasks"]) % 2 == 0:
                out.append(self.ref(self.take(ln), ln))
            else:
                out.append(self.alt(bytes(65 + (len(self.t["alt"]) + i) % 26 for i in range(ln))))
        return out

    def chain(self, n, ln=5):
        """n substitutions in a row on one source: copy, then n x (literal, copy) -> tasks of the literals"""
        sp = self.take((n + 1) * (ln + 1))
        self.ref(sp, ln)
        lits = []
        for k in range(n):
            lits.append(self.alt(bytes([97 + k])))
            self.ref(sp + (k + 1) * (ln + 1), ln)
        return lits

    def filler_bytes(self, n, piece=700):
        """reference copies of at most `piece` bytes, n bytes in all"""
        while n:
            k = min(n, piece)
            self.ref(self.take(k), k)
            n -= k

    def triple(self, l1, byte, l2, resume=1, lit=1):
        """copy, literal, copy that goes on `resume` residues behind the first one's end -> (task of the literal, of the closing copy)"""
        sp = self.take(l1 + resume + l2)
        self.ref(sp, l1)
        i = self.alt(bytes([byte + k for k in range(lit)]))
        j = self.ref(sp + l1 + resume, l2)
        return i, j

    def pair(self, l1, l2, l3, b1=ord("a"), b2=ord("b")):
        """two substitutions in a row (the dense image's five-part word) -> tasks of the two literals"""
        sp = self.take(l1 + l2 + l3 + 2)
        self.ref(sp, l1)
        i = self.alt(bytes([b1]))
        self.ref(sp + l1 + 1, l2)
        j = self.alt(bytes([b2]))
        self.ref(sp + l1 + 1 + l2 + 1, l3)
        return i, j

    def end_hap(self):
        self.hap_tx_begin.append(len(self.tx))

    # ---- the finished stream ----
    def res_len(self, t):
        return t["cur"] + t["extra"]

    def arena_len(self, t):
        return self.res_len(t) + (t["hlen"] + 1 if t["hlen"] else 0)

    def arrays(self):
        if self.hap_tx_begin[-1] != len(self.tx):
            self.end_hap()
        tb, ab, code, sp, ln, sr, alt = [0], [0], [], [], [], [], bytearray()
        for t in self.tx:
            for c, s, l, r in t["tasks"]:
                code.append(c); sp.append(s); ln.append(l); sr.append(r)
            alt += t["alt"]
            tb.append(len(code)); ab.append(len(alt))
        a = [self.hap_tx_begin, [t["off"] for t in self.tx], [t["ref_len"] for t in self.tx], [self.res_len(t) for t in self.tx], tb, ab,
             code, sp, ln, sr, np.frombuffer(bytes(alt), dtype=np.uint8)]
        if self.fasta:
            a += [[t["hoff"] for t in self.tx], [t["hlen"] for t in self.tx]]
        return a

    def reference(self):
        """(proteome, header table or None)"""
        return self.prot, (np.frombuffer(bytes(self.headers), dtype=np.uint8) if self.fasta else None)

    def want_tx(self, t):
        out = np.full(self.res_len(t), DOT, dtype=np.uint8)
        ref = self.prot[t["off"]:t["off"] + t["ref_len"]]
        ta = np.frombuffer(bytes(t["alt"]), dtype=np.uint8)
        for c, s, l, r in t["tasks"]:
            src = ref if c == 0 else ta
            assert c in (0, 1) and s + l <= src.size and r + l <= out.size, "the plain rule has no word for this Task: an error case"
            out[r:r + l] = src[s:s + l]
        if t["hlen"]:
            out = np.concatenate([np.frombuffer(t["header"], dtype=np.uint8), out, np.frombuffer(b"\n", dtype=np.uint8)])
        return out

    def want(self):
        """expected bytes of every haplotype"""
        self.arrays()
        hb = self.hap_tx_begin
        return [np.concatenate([self.want_tx(t) for t in self.tx[hb[h]:hb[h + 1]]] + [np.zeros(0, np.uint8)]) for h in range(len(hb) - 1)]

    # ---- positions ----
    def tx_base(self, u):
        return sum(self.arena_len(t) for t in self.tx[:u])

    def task_tx(self, i):
        for u, t in enumerate(self.tx):
            if i < len(t["tasks"]):
                return u, i
            i -= len(t["tasks"])
        raise IndexError

    def task_pos(self, i):
        """arena offset of the first result byte of Task i"""
        u, k = self.task_tx(i)
        return self.tx_base(u) + self.tx[u]["hlen"] + self.tx[u]["tasks"][k][3]

    def tile_items(self, K):
        """per tile: [(transcript, task or None)]"""
        tiles, g = [], 0
        for u, t in enumerate(self.tx):
            if u % K == 0:
                tiles.append([])
            if not t["tasks"]:
                tiles[-1].append((u, None))
            for _ in t["tasks"]:
                tiles[-1].append((u, g)); g += 1
        return tiles or [[]]

    def item_of(self, task, K):
        """(tile, item inside it, items of the tile) of a Task"""
        for ti, items in enumerate(self.tile_items(K)):
            for j, (_, g) in enumerate(items):
                if g == task:
                    return ti, j, len(items)
        raise IndexError(task)

    def item_of_tx(self, u, K):
        """... of an empty transcript's item"""
        for ti, items in enumerate(self.tile_items(K)):
            for j, (uu, g) in enumerate(items):
                if uu == u and g is None:
                    return ti, j, len(items)
        raise IndexError(u)


def _done(c, K, kernels=(6, 7), **kw):
    c.K = list(K) if isinstance(K, (list, tuple)) else [K]
    c.kernels = kernels
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    c.arrays()
    return c


def _lanes(c, task, K, kernels):
    """where every kernel's parse emits the item of `task`"""
    ti, j, n = c.item_of(task, K)
    return {k: emitted_at(j, n, k) for k in kernels}


# ================================================================== window seams
def _snv_k1(j, n_items=130, l1=3, l2=4):
    """one long transcript = one tile: the triple's literal is item j"""
    c = Case(seed=j)
    c.open()
    c.mixed(j - 1)
    lit, close = c.triple(l1, ord("a") + j % 26, l2)
    c.mixed(n_items - (j + 2))
    c.tail(3)
    assert c.item_of(lit, 1) == (0, j, n_items) and c.item_of(close, 1) == (0, j + 1, n_items)
    c.reach = dict(lit=j, close=_lanes(c, close, 1, (6, 7, 9)), first=_lanes(c, lit - 1, 1, (6, 7, 9)))
    return _done(c, 1, (6, 7, 9))


for _j in list(range(56, 69)) + list(range(112, 127)):
    case("window", f"snv_literal_is_item_{_j:03d}_of_a_one_transcript_tile")(lambda j=_j: _snv_k1(j))


def _k64(kind, j):
    """a tile of 64 transcripts of two items each; one of them holds a substitution, a pair or a chain of four whose first literal is item j
    of the tile: the window line falls inside a multi-transcript tile"""
    c = Case(seed=100 + j + len(kind))
    u_special, lits = (j - 1) // 2, None
    for u in range(70):
        c.open(off=37 * u % 4000, ref_len=3000)
        if u == u_special:
            c.mixed(j - 1 - 2 * u, ln=22)
            if kind == "snv":
                lit, close = c.triple(5, ord("a") + j % 26, 6)
                lits = [lit]
            elif kind == "pair":
                lits = list(c.pair(3, 4, 5))
            else:
                lits = c.chain(4)
            close = lits[-1] + 1
        else:
            c.mixed(2, ln=22 + u % 7)
        if u % 9 == 0:
            c.end_hap()
    ti, item, n = c.item_of(lits[0], 64)
    assert (ti, item) == (0, j) and n > 128
    c.reach = dict(lit=j, close=_lanes(c, close, 64, (6, 7, 9)))
    return _done(c, 64, (6, 7, 9))


for _j in range(56, 69):
    case("window", f"snv_literal_is_item_{_j:03d}_of_a_tile_of_64_transcripts")(lambda j=_j: _k64("snv", j))
    case("window", f"pair_first_literal_is_item_{_j:03d}_of_a_tile_of_64_transcripts")(lambda j=_j: _k64("pair", j))
for _j in range(50, 68):
    case("window", f"chain_of_four_from_item_{_j:03d}_of_a_tile_of_64_transcripts")(lambda j=_j: _k64("chain", j))


def _pair_k1(j, n_items=132):
    """the FIRST literal of two substitutions in a row is item j: the five-part word closes at item j + 3"""
    c = Case(seed=200 + j)
    c.open()
    c.mixed(j - 1)
    l1, l2 = c.pair(3, 4, 5)
    c.mixed(n_items - (j + 4))
    assert c.item_of(l1, 1) == (0, j, n_items) and c.item_of(l2, 1) == (0, j + 2, n_items)
    c.reach = dict(lit=j, close=_lanes(c, l2 + 1, 1, (6, 7, 9)), first=_lanes(c, l1 - 1, 1, (6, 7, 9)))
    return _done(c, 1, (6, 7, 9))


for _j in list(range(53, 69)) + list(range(109, 127)):
    case("window", f"pair_first_literal_is_item_{_j:03d}")(lambda j=_j: _pair_k1(j))


def _chain_k1(j, n_sub=6, n_items=140):
    """six substitutions in a row, the first literal is item j: the dense parse pairs them two by two FROM THE FIRST, which a window knows
    of the one before it only through the carried `second` bits; the wave parse fuses each with the copy the one before it closed on"""
    c = Case(seed=250 + j)
    c.open()
    c.mixed(j - 1, ln=22)                               # (22 bytes: the chain's short words still leave a row at most 64 descriptors)
    lits = c.chain(n_sub)
    c.mixed(n_items - (j + 2 * n_sub), ln=22)
    assert [c.item_of(g, 1)[1] for g in lits] == [j + 2 * k for k in range(n_sub)] and c.item_of(lits[0], 1)[2] == n_items
    c.reach = dict(lit=j, closes={k: [emitted_at(j + 2 * i + 1, n_items, k) for i in range(n_sub)] for k in (6, 7, 9)})
    return _done(c, 1, (6, 7, 9))


for _j in list(range(46, 68)) + list(range(104, 126)):
    case("window", f"chain_of_six_substitutions_from_item_{_j:03d}")(lambda j=_j: _chain_k1(j))


def _tile_of(n):
    """a tile of exactly n items that ends in a triple and a '.' tail: the `last` decision and the mask of active lanes"""
    c = Case(seed=300 + n)
    c.open()
    c.mixed(n - 3)
    lit, close = c.triple(2, ord("q"), 3)
    c.tail(5)
    assert c.item_of(close, 1) == (0, n - 1, n)
    c.reach = dict(n_items=n, windows={k: len(windows(n, k)) for k in (6, 7, 9)})
    return _done(c, 1, (6, 7, 9))


for _n in (1, 2, 3, 61, 62, 63, 64, 65, 66, 119, 120, 121, 122, 123, 124, 125, 126):
    case("window", f"tile_of_exactly_{_n:03d}_items")(lambda n=_n: _tile_of(max(n, 3)) if n >= 3 else _tile_small(n))


def _tile_small(n):
    c = Case(seed=390 + n)
    c.open()
    c.fillers(n, ln=7)
    c.tail(2)
    c.reach = dict(n_items=n)
    return _done(c, 1, (6, 7, 9))


def _kind_at(kind, j):
    """item j of the tile is: a zero-length Task, a Task behind a gap, a transcript's first item, an empty transcript, a last item with a tail"""
    c = Case(seed=400 + j)
    c.open(ref_len=4000)
    if kind in ("zero", "gap", "tail"):
        c.fillers(j)
        if kind == "zero":
            g = c.ref(c.take(0), 0)
        elif kind == "gap":
            c.gap(7)
            g = c.fillers(1)[0]
        else:
            g = c.fillers(1)[0]
            c.tail(9)
            c.open(off=100, ref_len=500)
        c.fillers(70 - j)
        where = c.item_of(g, 8)
    else:
        c.fillers(j)
        u = c.open(off=200, ref_len=900)
        if kind == "first":
            c.gap(4)
            g = c.fillers(1)[0]
            c.fillers(3)
            where = c.item_of(g, 8)
        else:
            c.tail(11)                                 # (no Tasks: eleven '.')
            where = c.item_of_tx(u, 8)
        c.open(off=300, ref_len=900)
        c.fillers(70 - j)
    assert where[0] == 0 and where[1] == j, (kind, j, where)
    c.reach = dict(kind=kind, item=j, at={k: emitted_at(j, where[2], k) for k in (6, 7, 9)})
    return _done(c, 8, (6, 7, 9))


for _kind in ("zero", "gap", "first", "empty", "tail"):
    for _j in range(59, 67):
        case("window", f"item_{_j:03d}_is_{_kind}")(lambda kind=_kind, j=_j: _kind_at(kind, j))


# ================================================================== fusion rules
def _fuse_lens(l1, l2):
    c = Case(prot_len=8192, seed=500 + l1 + 3 * l2)
    c.open()
    c.fillers(2)
    c.triple(l1, ord("m"), l2)
    c.fillers(2)
    c.triple(l1, ord("n"), l2)                         # (twice: the second one sits at another offset inside its row)
    fuses = l1 <= ROWS_FUSE_LEN and l2 <= ROWS_FUSE_LEN
    c.reach = dict(fuses=fuses)
    return _done(c, 1, (6, 7, 9) if max(l1, l2) < 600 else (6, 7))


for _l1, _l2 in [(0, 5), (1, 5), (1023, 5), (1024, 5), (1025, 5), (5, 0), (5, 1), (5, 1023), (5, 1024), (5, 1025), (1023, 1023), (1024, 1024), (0, 0), (0, 1023), (0, 1024)]:
    case("fusion", f"copies_of_{_l1}_and_{_l2}_beside_the_literal")(lambda a=_l1, b=_l2: _fuse_lens(a, b))


def _pair_lens(l1, l2, l3):
    c = Case(seed=600 + l1 + 2 * l2 + 3 * l3)
    c.open()
    c.fillers(3)
    c.pair(l1, l2, l3)
    c.fillers(2)
    c.pair(l1, l2, l3)
    c.reach = dict(pairs=max(l1, l2, l3) <= SNV5_MAX_LEN)
    return _done(c, 1, (6, 7, 9))


for _l in [(31, 31, 31), (32, 5, 5), (5, 32, 5), (5, 5, 32), (31, 5, 5), (5, 31, 5), (5, 5, 31), (0, 0, 0), (0, 5, 0), (32, 32, 32)]:
    case("fusion", "pair_with_copies_of_%d_%d_%d" % _l)(lambda l=_l: _pair_lens(*l))


@case("fusion")
def second_copy_resumes_at_src_plus_0_1_2():
    c = Case(seed=700)
    c.open()
    for resume in (1, 0, 2, 1):                        # only `1` fuses
        c.fillers(1)
        c.triple(6, ord("r"), 7, resume=resume)
    return _done(c, 1, (6, 7, 9))


@case("fusion")
def literal_of_one_and_of_two_bytes():
    c = Case(seed=701)
    c.open()
    for lit in (1, 2, 1, 2):
        c.fillers(1)
        c.triple(6, ord("s"), 7, lit=lit)
    return _done(c, 1, (6, 7, 9))


@case("fusion")
def triple_at_the_very_start_of_the_proteome():
    """an empty first copy: the run is the literal's residue - 1, so the closing copy must start at source 1 or later"""
    c = Case(seed=702)
    c.open(off=0)
    c.alt(b"x")
    c.ref(1, 9)                                        # source 1: fuses, the run starts at 0
    c.open(off=0)
    c.alt(b"y")
    c.ref(0, 9)                                        # source 0: there is no residue in front of it -- no fusion
    c.open(off=0)
    c.ref(0, 0)
    c.alt(b"z")
    c.ref(1, 9)                                        # an EMPTY held copy at source 0
    assert c.tx[0]["off"] + c.tx[0]["tasks"][1][1] == 1 and c.tx[1]["off"] + c.tx[1]["tasks"][1][1] == 0
    return _done(c, [1, 64], (6, 7, 9))


@case("fusion")
def triple_broken_by_a_gap():
    c = Case(seed=703)
    c.open()
    sp = c.take(40)
    c.ref(sp, 5); c.gap(1); c.alt(b"g"); c.ref(sp + 6, 5)           # gap in front of the literal
    sp = c.take(40)
    c.ref(sp, 5); c.alt(b"h"); c.gap(1); c.ref(sp + 6, 5)           # gap in front of the closing copy
    sp = c.take(40)
    c.gap(2); c.ref(sp, 5); c.alt(b"i"); c.ref(sp + 6, 5)           # gap in front of the first copy: fuses
    return _done(c, 1, (6, 7, 9))


@case("fusion")
def triple_broken_by_a_transcript_boundary():
    c = Case(seed=704)
    c.open(off=10, ref_len=100)
    c.ref(0, 5); c.alt(b"k")
    c.open(off=10, ref_len=100)
    c.ref(6, 5)                                                      # continues the source of the transcript before it: not its run
    c.open(off=10, ref_len=100)
    c.ref(0, 5)
    c.open(off=10, ref_len=100)
    c.alt(b"l"); c.ref(6, 5)                                         # the literal opens its own transcript
    assert c.item_of(2, 64)[1] == 2
    return _done(c, [64, 1, 2], (6, 7, 9))


# ================================================================== immediates and alt bytes
def _imm(n, align):
    c = Case(seed=800 + 4 * n + align)
    c.open()
    c.fillers(1)
    c.alt(bytes(range(65, 65 + 8 + align)))            # (a payload run in front: the next alt byte sits at offset 8 + align of the tile's)
    c.fillers(1, ln=11)
    i = c.alt(bytes(range(97, 97 + n)))
    c.fillers(1, ln=5)
    c.alt(bytes(range(48, 48 + n)))
    assert c.t["tasks"][3][1] % 4 == align and c.t["tasks"][3][2] == n
    c.reach = dict(imm=n <= IMM_MAX_BYTES, align=align)
    return _done(c, 1, (6, 7, 9))


for _n in (1, 4, 5, 6):
    for _a in range(4):
        case("immediates", f"payload_of_{_n}_bytes_at_alignment_{_a}")(lambda n=_n, a=_a: _imm(n, a))


def _alt_total(total):
    """the tile's alt bytes: 511, 512 (in LDS), 513 (from memory).  The first Task's 5-byte payload ends on the tile's LAST alt byte; a second
    tile's alt bytes lie behind it, so its unaligned 8-byte load stays inside the array whatever is allocated behind that"""
    c = Case(seed=900 + total)
    c.open()
    rng = np.random.default_rng(total)
    tape = AA[rng.integers(0, 20, size=total)].tobytes()
    c.t["alt"] += tape
    c.raw(1, total - 5, 5, 0)
    at = 0
    for n in (1, 3, 5, 6, 2, 4, 5, 40, 1, 5):
        c.fillers(1, ln=4)
        c.raw(1, at, n, c.t["cur"]); at += n + 1
    c.fillers(1, ln=4)
    c.raw(1, total - 1, 1, c.t["cur"])
    c.open(off=50, ref_len=300)
    c.fillers(1)
    c.alt(b"tail-of-the-alt-array")
    assert len(c.tx[0]["alt"]) == total and c.tx[0]["tasks"][0][1] + 5 == total
    c.reach = dict(in_lds=total <= ROWS_ALT_LDS)
    return _done(c, 1, (6, 7, 9))


for _t in (511, 512, 513):
    case("immediates", f"tile_alt_total_{_t}")(lambda t=_t: _alt_total(t))


# ================================================================== rows and long runs
LINE = 2 * ROW_BYTES
RUNS = dict(header=(0, 20), gap=(20, 30), task=(50, 40), tail=(90, 25), lf=(115, 1))          # (offset inside the record, length)


def _run_at_line(kind, rel):
    """a FASTA record [header 20][gap 30][task 40][tail 25][line feed] placed so that run `kind` ends on / starts on / straddles the row line
    at 2048 by one byte on either side"""
    off, ln = RUNS[kind]
    start = {"ends_on": LINE - ln, "starts_on": LINE, "one_before": LINE - 1, "one_past": LINE + 1 - ln}[rel]
    c = Case(fasta=True, seed=1000 + off + len(rel))
    c.open()                                            # (no header)
    c.filler_bytes(start - off)
    u = c.open(off=500, ref_len=2000, header="R" * 18)
    assert c.t["hlen"] == 20
    c.gap(30)
    c.ref(c.take(40), 40)
    c.tail(25)
    c.open(off=70, ref_len=800, header="next")
    c.fillers(2, ln=30)
    b = c.tx_base(u)
    s, e = b + off, b + off + ln
    assert {"ends_on": e == LINE, "starts_on": s == LINE, "one_before": s == LINE - 1 and e > LINE, "one_past": e == LINE + 1 and s < LINE}[rel], (s, e)
    c.reach = dict(kind=kind, rel=rel)
    return _done(c, [2, 1], (6, 7))


for _kind in RUNS:
    for _rel in ("ends_on", "starts_on", "one_before", "one_past"):
        if _kind == "lf" and _rel in ("one_before", "one_past"):
            continue                                    # (one byte: it cannot straddle)
        case("rows", f"{_kind}_run_{_rel}_a_row_line")(lambda k=_kind, r=_rel: _run_at_line(k, r))


def _plain_task_at_line(rel, ln=100):
    """the PLAIN window (no gap, no tail, no FASTA text in it): one Task's run against the row line at 2048"""
    start = {"ends_on": LINE - ln, "starts_on": LINE, "one_before": LINE - 1, "one_past": LINE + 1 - ln}[rel]
    c = Case(seed=1100 + len(rel))
    c.open()
    c.filler_bytes(start, piece=90)
    g = c.ref(c.take(ln), ln)
    c.filler_bytes(1500, piece=90)
    assert c.task_pos(g) == start and all(t["extra"] == 0 for t in c.tx)
    return _done(c, 1, (6, 7))


for _rel in ("ends_on", "starts_on", "one_before", "one_past"):
    case("rows", f"plain_window_task_{_rel}_a_row_line")(lambda r=_rel: _plain_task_at_line(r))


@case("rows")
def plain_window_last_run_of_a_long_tile_ends_on_the_line_the_next_tile_starts_on():
    """Tile 0: four windows of Tasks, its last run ends exactly on the row line at 8192 (no tail: every window is plain).  Tile 1 starts on
    that line and is one window.  The row's cover word is tile 1's to write: a parse that lets the run ENDING on a line claim it writes it
    from tile 0's last window, long after tile 1 wrote the true one."""
    c = Case(seed=1150)
    c.open()
    c.filler_bytes(8 * ROW_BYTES - 29, piece=40)
    g = c.ref(c.take(29), 29)
    c.open(off=11, ref_len=3000)
    c.filler_bytes(1500, piece=50)
    n0 = len(c.tx[0]["tasks"])
    assert c.task_pos(g) + 29 == 8 * ROW_BYTES == c.tx_base(1) and len(windows(n0, 6)) >= 4 and len(windows(len(c.tx[1]["tasks"]), 6)) == 1
    assert n0 <= ROWS_TILE_SLOTS and all(t["extra"] == 0 for t in c.tx)
    return _done(c, 1, (6, 7), two_pass=False)


@case("rows")
def general_window_one_lane_whose_gap_task_and_tail_cover_three_row_lines():
    c = Case(seed=1160)
    c.open()
    c.filler_bytes(1000)
    c.gap(600)                                          # 1000 .. 1600: line 1024
    g = c.ref(c.take(900), 900)                         # 1600 .. 2500: line 2048
    c.tail(1000)                                        # 2500 .. 3500: line 3072
    assert c.task_pos(g) == 1600 and c.arena_len(c.t) == 3500
    return _done(c, 1, (6, 7))


def _long_run(kind, ln, at):
    """a run of ln bytes (more than 1 KiB: the parse's `slow` form cuts it into pieces of PIECE_MAX) that starts at offset `at` of a row"""
    c = Case(prot_len=8192, seed=1200 + ln + at)
    c.open()
    c.filler_bytes(ROW_BYTES + at)
    if kind == "task":
        g = c.ref(c.take(ln), ln)
        s = c.task_pos(g)
    elif kind == "payload":
        rng = np.random.default_rng(ln)
        g = c.alt(AA[rng.integers(0, 20, size=ln)].tobytes())
        s = c.task_pos(g)
    elif kind == "gap":
        s = c.tx_base(0) + c.t["cur"]
        c.gap(ln)
        c.fillers(1)
    else:
        s = c.tx_base(0) + c.t["cur"]
        c.tail(ln)
    c.open(off=9, ref_len=500)
    c.fillers(2, ln=20)
    assert s == ROW_BYTES + at and ln >= ROW_BYTES
    c.reach = dict(pieces=-(-ln // PIECE_MAX), lines=(s + ln - 1) // ROW_BYTES - (s - 1) // ROW_BYTES if s else 0)
    return _done(c, [1, 2], (6, 7))


for _ln in (1024, 1025, 2047, 2048, 2049, 4095):
    for _at in (0, 1, 1023):
        case("rows", f"copy_of_{_ln}_bytes_at_row_offset_{_at}")(lambda ln=_ln, at=_at: _long_run("task", ln, at))
for _kind in ("payload", "gap", "tail"):
    for _ln, _at in ((1025, 1023), (2048, 1), (4095, 0)):
        case("rows", f"{_kind}_of_{_ln}_bytes_at_row_offset_{_at}")(lambda k=_kind, ln=_ln, at=_at: _long_run(k, ln, at))


def _fused_2047(at):
    c = Case(prot_len=8192, seed=1300 + at)
    c.open()
    c.filler_bytes(ROW_BYTES + at)
    lit, close = c.triple(ROWS_FUSE_LEN, ord("w"), ROWS_FUSE_LEN)
    c.fillers(2)
    s = c.task_pos(lit) - ROWS_FUSE_LEN
    assert s == ROW_BYTES + at and (s + 2046) // ROW_BYTES > s // ROW_BYTES
    return _done(c, 1, (6, 7))


for _at in (0, 1, 2, 1023):
    case("rows", f"fused_word_of_2047_bytes_at_row_offset_{_at}")(lambda at=_at: _fused_2047(at))


def _arena_of(n):
    c = Case(seed=1400 + n)
    c.open()
    c.filler_bytes(n - 100, piece=300)
    c.triple(40, ord("e"), 59)
    assert c.arena_len(c.t) == n
    return _done(c, 1, (6, 7))


for _n in (1023, 1024, 1025, 2048):
    case("rows", f"arena_of_exactly_{_n}_bytes")(lambda n=_n: _arena_of(n))


# ================================================================== tiles and haplotypes
def _cohort(n_tx, seed, fasta=False, hap_sizes=None):
    """n_tx short transcripts of every shape, in haplotypes of irregular size: empty ones first, last and three in a row"""
    rng = np.random.default_rng(seed)
    c = Case(prot_len=6000, fasta=fasta, seed=seed)
    sizes = hap_sizes or [0, 3, 5, 0, 0, 0, 1, 7, 2, 11, 4, 0, 6, 13, 1, 1, 9]
    ends, at, k = [], 0, 0                              # the transcript behind which every haplotype ends
    while at < n_tx:
        at += sizes[k % len(sizes)]; k += 1
        ends.append(min(at, n_tx))
    for u in range(n_tx):
        while ends and ends[0] == u:
            ends.pop(0)
            c.end_hap()
        shape = u % 7
        hdr = None if not fasta or u % 11 == 5 else "T%d_%s" % (u, "x" * (u % 13))
        c.open(off=int(rng.integers(0, 5000)), ref_len=900, header=hdr)
        if shape == 0:                                  # (sizes: about 25 result bytes per descriptor, so that a wave image takes every row)
            c.tail(25 + u % 5)                          # no Tasks
        elif shape == 1:
            c.triple(10 + u % 9, 97 + u % 26, 14 + u % 8)
        elif shape == 2:
            c.fillers(1 + u % 4, ln=20 + u % 6); c.tail(18 * (u % 2))
        elif shape == 3:
            c.pair(8 + u % 5, 9 + u % 4, 10 + u % 6)
        elif shape == 4:
            c.gap(16 + u % 4); c.fillers(1, ln=30); c.alt(bytes(range(65, 65 + 1 + u % 9))); c.fillers(1, ln=30)
        elif shape == 5:
            c.triple(13, 97 + u % 26, 14); c.triple(12, 98 + u % 20, 12); c.tail(17)
        else:
            c.ref(c.take(0), 0); c.fillers(2, ln=40 + u % 30)
    c.end_hap()
    c.end_hap(); c.end_hap()                            # two empty haplotypes last
    return c


def _hap_reach(c, K):
    hb = c.hap_tx_begin
    mid = [h for h in range(len(hb) - 1) if hb[h] % K]
    three = [h for h in range(len(hb) - 3) if hb[h] == hb[h + 1] == hb[h + 2] == hb[h + 3] and hb[h] % K]
    return mid, three


def _sweep(n_tx, Ks, fasta=False):
    c = _cohort(n_tx, 1500 + n_tx, fasta)
    hb = c.hap_tx_begin
    assert hb[0] == hb[1] == 0 and hb[-1] == hb[-2] == hb[-3] == n_tx            # empty haplotypes first and last
    for K in Ks:
        mid, three = _hap_reach(c, K)
        assert K == 1 or mid, K                                                  # haplotypes that begin in the middle of a tile
    assert any(_hap_reach(c, K)[1] for K in Ks if K > 1) or Ks == [1]            # three empty ones in a row mid-tile
    c.reach = dict(rem={K: n_tx % K for K in Ks})
    return _done(c, Ks, (6, 7, 9))


case("tiles", "sweep_of_K_over_192_transcripts")(lambda: _sweep(192, [1, 2, 31, 32, 33, 63, 64]))
case("tiles", "n_tx_is_one_more_than_a_multiple_of_K")(lambda: _sweep(193, [2, 32, 64, 3, 48]))
case("tiles", "n_tx_is_one_less_than_a_multiple_of_K")(lambda: _sweep(191, [2, 32, 64, 3, 48]))
case("tiles", "n_tx_against_31_33_63")(lambda: _sweep(189, [31, 33, 63]))          # 189 = 3 * 63 = 6 * 31 + 3 = 5 * 33 + 24
case("tiles", "n_tx_is_K_plus_minus_one_for_31_33_63")(lambda: _sweep(64, [31, 33, 63, 64]))            # 64 = 2 * 31 + 2 = 33 + 31 = 63 + 1
case("tiles", "fasta_sweep_of_K")(lambda: _sweep(150, [1, 2, 31, 32, 33, 48, 64], fasta=True))


@case("tiles")
def n_tx_remainders_are_0_1_and_K_minus_1():
    """(the three cases above, from the numbers alone)"""
    assert 192 % 64 == 192 % 32 == 192 % 2 == 0 and 193 % 64 == 193 % 32 == 193 % 2 == 193 % 3 == 193 % 48 == 1
    assert 191 % 64 == 63 and 191 % 32 == 31 and 191 % 2 == 1 and 191 % 3 == 2 and 191 % 48 == 47
    assert 189 % 63 == 0 and 64 % 63 == 1 and 64 % 33 == 31 and 192 % 31 == 6 and 192 % 33 == 27 and 64 % 31 == 2
    return _sweep(65, [64, 33, 32, 22, 13])            # 65 = 64 + 1 = 2 * 33 - 1 = 2 * 32 + 1 = 3 * 22 - 1 = 5 * 13


@case("tiles")
def a_tile_made_only_of_empty_transcripts():
    c = Case(seed=1600)
    for u in range(12):
        c.open(off=5 * u, ref_len=100)
        if 4 <= u < 8:
            c.tail(3 + u)
        else:
            c.fillers(2, ln=6); c.tail(1)
        if u in (2, 5, 6):
            c.end_hap()
    assert all(g is None for _, g in c.tile_items(4)[1]) and len(c.tile_items(4)[1]) == 4
    return _done(c, [4, 2, 1], (6, 7, 9))


@case("tiles")
def every_transcript_is_empty():
    c = Case(seed=1601)
    for u in range(9):
        c.open(off=0, ref_len=10)
        c.tail(1 + u * 300)
        if u % 4 == 1:
            c.end_hap()
    assert c.n_tasks() == 0
    return _done(c, [1, 4, 64], (6, 7))


@case("tiles")
def a_stream_without_a_single_transcript():
    c = Case(seed=1602)
    c.end_hap(); c.end_hap(); c.end_hap()
    assert not c.tx and len(c.hap_tx_begin) == 4
    return _done(c, [1, 64], (6, 7))


# ================================================================== the two-pass form
def _tile_of_desc(n, src64=False):
    """one tile (K = 1) of exactly n descriptors: n copies of 20 bytes that fuse with nothing, no gap, no tail"""
    c = Case(seed=1700 + n)
    c.open()
    c.fillers(n, ln=20)
    c.open(off=3, ref_len=200)
    c.fillers(3, ln=20)
    assert len(c.tx[0]["tasks"]) == n and c.tx[0]["extra"] == 0
    return _done(c, 1, (6, 7), two_pass=n > ROWS_TILE_SLOTS, src64=src64, onecall_fell_back=n > ROWS_TILE_SLOTS)


for _n in (255, 256, 257, 600):
    case("two_pass", f"tile_of_{_n}_descriptors")(lambda n=_n: _tile_of_desc(n))
    case("two_pass", f"tile_of_{_n}_descriptors_with_64_bit_sources")(lambda n=_n: _tile_of_desc(n, True))


@case("two_pass")
def the_seams_of_the_window_with_64_bit_sources():
    c = _snv_k1(61)
    return _done(c, 1, (6, 7), src64=True)


@case("two_pass")
def a_sweep_of_K_with_64_bit_sources():
    c = _cohort(100, 1750)
    return _done(c, [1, 32, 64], (6, 7), src64=True)


@case("two_pass")
def long_runs_and_payloads_with_64_bit_sources():
    c = _long_run("payload", 2049, 1023)
    return _done(c, 1, (6, 7), src64=True)


# ================================================================== the cutter
def _rows_of(per_row, n_rows):
    """n_rows rows of exactly per_row descriptors each, every row's first descriptor starting on its line; one transcript per row (K = 1)"""
    c = Case(seed=1800 + per_row)
    for r in range(n_rows):
        c.open(off=(17 * r) % 3000, ref_len=3000)
        small = ROW_BYTES // per_row
        for k in range(per_row):
            ln = small if k + 1 < per_row else ROW_BYTES - small * (per_row - 1)
            c.ref(c.take(ln), ln)
        assert c.arena_len(c.t) == ROW_BYTES and c.tx_base(r) == r * ROW_BYTES
    return c


@case("cutter")
def rows_of_64_descriptors():
    c = _rows_of(64, 5)

    def check(case_, packed, kernel):
        if kernel == 6:
            n = (packed.chunks[:, 1] >> np.uint64(48)) & np.uint64(0x7FF)
            assert list(n) == [64] * 5
    return _done(c, 1, (6, 7), check_image=check, cut_emit_pass=False)


@case("cutter")
def a_row_of_65_descriptors_is_not_a_wave_image():
    c = _rows_of(64, 3)
    c.open(off=0, ref_len=3000)
    for k in range(65):
        ln = 15 if k < 64 else ROW_BYTES - 15 * 64
        c.ref(c.take(ln), ln)
    assert c.arena_len(c.t) == ROW_BYTES
    return _done(c, 1, (6, 7), refused={6: ERR_UNSUPPORTED})


@case("cutter")
def rows_of_33_descriptors_give_one_row_chunks_and_a_reload():
    """70 rows of 33 descriptors: two rows would be 66, so every chunk is one row -- more than 54 chunks out of one load of 64 rows, where the
    walk must reload (`cur + max_rows > 63`)"""
    c = _rows_of(33, 70)

    def check(case_, packed, kernel):
        if kernel == 6:
            dst = packed.chunks[:, 1] & np.uint64((1 << 48) - 1)
            assert packed.chunks.shape[0] == 70 and list(dst // np.uint64(ROW_BYTES)) == list(range(70))
    return _done(c, 1, (6, 7), check_image=check, cut_emit_pass=False)


def chunk_pad_for(out_bytes, n_items, kernel):
    """build_rows.h: rows_chunk_pad_for -- the chunk slots a 640-row segment has in the cutter's padded table"""
    max_rows, max_desc = (ROWS_MAX_DENSE, CHUNK_TASKS_DEEP) if kernel == 7 else (ROWS_MAX_WAVE, CHUNK_TASKS_WAVE)
    rows = max_desc * (out_bytes // n_items) // ROW_BYTES if n_items else max_rows
    rows = min(max(rows, 1), max_rows)
    pad = (3 * ((ROWS_SEG + rows - 1) // rows) // 2 + 31) & ~31
    return min(max(pad, ROWS_CHUNK_PAD), ROWS_SEG)


@case("cutter")
def a_segment_with_more_chunks_than_its_padded_slots_runs_the_emitting_pass():
    """100 rows of 33 descriptors -- 100 one-row wave chunks -- in front of 430 KiB of '.': the stream as a whole is sparse (more than 160
    result bytes per item), so a segment has the floor of 96 slots, and segment 0 holds 100 + 43 chunks"""
    c = _rows_of(33, 100)
    c.open(off=0, ref_len=10)
    c.tail(430 * ROW_BYTES)
    out_bytes, n_items = 530 * ROW_BYTES, c.n_tasks()
    assert out_bytes // n_items >= 160 and chunk_pad_for(out_bytes, n_items, 6) == ROWS_CHUNK_PAD == chunk_pad_for(out_bytes, n_items, 7)
    assert out_bytes <= ROWS_SEG * ROW_BYTES and -(-430 * ROW_BYTES // PIECE_MAX) <= ROWS_TILE_SLOTS

    def check(case_, packed, kernel):
        assert (packed.chunks.shape[0] > ROWS_CHUNK_PAD) == (kernel == 6), packed.chunks.shape
    return _done(c, 1, (6, 7), check_image=check, two_pass=False, cut_emit_pass=True, onecall_fell_back=True)


def _sparse_after_three_dense_rows(n_rows, seed):
    """rows 0 .. 2 hold 64 descriptors between them and row 3 ten more, so the first wave chunk is three rows; everything behind is copies of
    1500 bytes: chunks of ten rows starting at rows 3, 13, .., 53 -- the one that starts at row 53 ends at row 63, the last row of the walk's
    first load of 64"""
    c = Case(prot_len=8192, seed=seed)
    c.open()
    for k in range(64):
        c.ref(c.take(48), 48)                           # 64 x 48 = 3072
    for k in range(10):
        c.ref(c.take(20), 20)
    assert c.t["cur"] == 3 * ROW_BYTES + 200
    left = n_rows * ROW_BYTES - c.t["cur"]
    k = 0
    while left:
        if k % 100 == 99:
            c.open(off=k % 50, ref_len=8000)            # (tiles of at most 174 descriptors)
        ln = min(1500, left)
        c.ref(c.take(ln), ln)
        left -= ln; k += 1
    return c


@case("cutter")
def a_wave_chunk_that_ends_on_the_last_row_of_a_load():
    c = _sparse_after_three_dense_rows(80, 1850)

    def check(case_, packed, kernel):
        if kernel == 6:
            rows = sorted(int(x) // ROW_BYTES for x in packed.chunks[:, 1] & np.uint64((1 << 48) - 1))
            assert rows[:8] == [0, 3, 13, 23, 33, 43, 53, 63], rows[:8]
    return _done(c, 1, (6, 7), check_image=check, cut_emit_pass=False)


@case("cutter")
def a_chunk_that_would_cross_a_multiple_of_640_rows():
    """641 rows of few, long copies: the chunk that starts at row 633 would run to 643 and is cut at 640 (ROWS_SEG)"""
    c = _sparse_after_three_dense_rows(ROWS_SEG + 1, 1851)

    def check(case_, packed, kernel):
        rows = sorted(int(x) // ROW_BYTES for x in packed.chunks[:, 1] & np.uint64((1 << 48) - 1))
        assert ROWS_SEG in rows and rows[-1] == ROWS_SEG
        if kernel == 6:
            assert rows[-3:] == [623, 633, ROWS_SEG], rows[-3:]                    # (633 + 10 = 643: cut at 640)
        full = max(b - a for a, b in zip(rows, rows[1:]))
        assert full == (ROWS_MAX_WAVE if kernel == 6 else ROWS_MAX_DENSE)         # sparse descriptors: chunks of the full ten / twelve rows
    return _done(c, 1, (6, 7), check_image=check, cut_emit_pass=False)


@case("cutter")
def a_dense_chunk_whose_twelfth_row_would_pass_1024_descriptors():
    """copies of 11 bytes back to back from byte 0: eleven rows hold exactly 1024 descriptors -- the most a dense chunk takes -- and twelve 1118"""
    c = Case(seed=1860)
    for u in range(20):
        c.open(off=7 * u, ref_len=5000)
        c.fillers(200, ln=11)
    assert 11 * ROW_BYTES == 11 * CHUNK_TASKS_DEEP and -(-12 * ROW_BYTES // 11) > CHUNK_TASKS_DEEP

    def check(case_, packed, kernel):
        if kernel == 7:
            rows = sorted(int(x) // ROW_BYTES for x in packed.chunks[:, 1] & np.uint64((1 << 48) - 1))
            assert rows[:3] == [0, 11, 22], rows[:3]
    return _done(c, 1, (7,), check_image=check)


# ================================================================== the one call's padded image
def _tiles_of(n_desc_per_tile, n_tiles, ln=17):
    c = Case(seed=1900 + n_desc_per_tile)
    for u in range(n_tiles):
        c.open(off=3 * u, ref_len=6000)
        c.fillers(n_desc_per_tile, ln=ln)
    return c


@case("onecall")
def a_chunk_whose_descriptors_span_two_tiles():
    """tiles (K = 1) of 100 descriptors of 17 bytes: a wave chunk holds at most 64 of them, so it ends in its first tile or in the next one"""
    c = _tiles_of(100, 200)
    assert len(c.tx) // 3 >= 64                          # (the one call keeps at least 64 tiles to a slice)

    def check(case_, packed, kernel):
        if kernel == 6:
            first = packed.chunks[:, 0] & np.uint64((1 << 42) - 1)
            n = (packed.chunks[:, 1] >> np.uint64(48)) & np.uint64(0x7FF)
            spans = (first + n - np.uint64(1)) // np.uint64(100) - first // np.uint64(100)
            assert int(spans.max()) == 1 and int(spans.min()) == 0
    return _done(c, 1, (6, 7), check_image=check, onecall_fell_back=False, slices=(2, 3))


@case("onecall")
def a_chunk_that_would_span_three_tiles_falls_back():
    """tiles of 20 descriptors: 60 to the row, so a chunk of one row spans four tiles -- the padded image cannot write that down"""
    c = _tiles_of(20, 200)

    def check(case_, packed, kernel):
        if kernel == 6:
            first = packed.chunks[:, 0] & np.uint64((1 << 42) - 1)
            n = (packed.chunks[:, 1] >> np.uint64(48)) & np.uint64(0x7FF)
            assert int(((first + n - np.uint64(1)) // np.uint64(20) - first // np.uint64(20)).max()) >= 2
    return _done(c, 1, (6,), check_image=check, onecall_fell_back=True, slices=(2, 3))


# ================================================================== tile images (kernel 9)
def _piece_literal(p, where):
    """a fused run of 80 bytes = five pieces of 16: the literal at position p of the first / the last piece"""
    c = Case(seed=2000 + p)
    c.open()
    c.fillers(2, ln=16)                                  # (the run starts on a piece line of the tile's result)
    l1 = p if where == "first" else 64 + p
    lit, close = c.triple(l1, ord("u"), 80 - l1 - 1)
    c.fillers(1)
    s = c.task_pos(lit) - l1
    assert s % PIECE_BYTES == 0 and (c.task_pos(lit) - s) // 16 == (0 if where == "first" else 4) and (c.task_pos(lit) - s) % 16 == p
    return _done(c, 1, (9, 6, 7))


for _p in range(16):
    case("tile_image", f"literal_at_position_{_p:02d}_of_the_first_piece")(lambda p=_p: _piece_literal(p, "first"))
    if _p < 15:
        case("tile_image", f"literal_at_position_{_p:02d}_of_the_last_piece")(lambda p=_p: _piece_literal(p, "last"))


def _piece_runs(ln):
    c = Case(seed=2100 + ln)
    c.open()
    for at in (0, 1, 15):
        c.fillers(1, ln=16 + at)
        c.ref(c.take(ln), ln)
        c.alt(bytes(range(65, 65 + ln)))
        c.gap(ln)
        c.fillers(1, ln=3)
    c.tail(ln)
    return _done(c, 1, (9, 6, 7))


for _ln in (15, 16, 17, 32, 33):
    case("tile_image", f"runs_of_{_ln}_bytes")(lambda ln=_ln: _piece_runs(ln))


def _tile_span(K, span):
    """K transcripts of 255 or 256 bytes whose result is `span` bytes in all (the K the statistics pick for them is one or two short of
    this: its slots hold the forced tile's pieces)"""
    c = Case(seed=2200 + span % 100)
    for u in range(K):
        c.open(off=11 * u, ref_len=7000)
        n = 256 if u < span - 255 * K else 255
        c.filler_bytes(n - 10, piece=123)
        c.triple(3, ord("v"), 6)
    c.open(off=1, ref_len=100)
    c.fillers(1)
    assert sum(c.arena_len(t) for t in c.tx[:K]) == span
    return c


@case("tile_image")
def a_tile_span_just_under_the_limit():
    return _done(_tile_span(64, TILE_SPAN_MAX), 64, (9,))


@case("tile_image")
def a_tile_span_just_over_the_limit_is_refused():
    return _done(_tile_span(64, TILE_SPAN_MAX + 1), 64, (9,), refused={9: ERR_UNSUPPORTED})


def tile_slots_for(c):
    """v2p_api.hip: stream_item_stats + rows_pick_k_tiles -- (the K the statistics pick, the piece slots they give a tile); a forced K keeps
    the slots"""
    import math
    d, l = [], []
    for t in c.tx:
        k = t["tasks"]
        nf = sum(1 for i in range(1, len(k) - 1) if k[i][0] == 1 and k[i][2] == 1 and k[i - 1][0] == 0 and k[i + 1][0] == 0)
        d.append((len(k) - 2 * nf if len(k) > 2 * nf else 1.0) + 1.0)
        l.append(float(c.arena_len(t)))
    dm, lm = sum(d) / len(d), sum(l) / len(l)
    dv, lv = max(sum(x * x for x in d) / len(d) - dm * dm, 0.0), max(sum(x * x for x in l) / len(l) - lm * lm, 0.0)
    z, lm1, lsd = 6.0, max(lm, 1.0), math.sqrt(lv)
    pm, psd = dm + (2.0 if c.fasta else 0.0) + lm1 / 16.0, math.sqrt(dv) + lsd / 16.0

    def k_for(m, sd, cap):
        x = (-z * sd + math.sqrt(z * z * sd * sd + 4.0 * m * cap)) / (2.0 * m)
        return math.floor(x * x)
    k = min(k_for(lm1, lsd, TILE_SPAN_MAX - 64.0), k_for(pm, psd, TILE_SLOTS_MAX - 16.0), 64.0)
    assert k >= 1.0
    need, sl = k * pm + z * psd * math.sqrt(k) + 16.0, 256
    while sl < TILE_SLOTS_MAX and sl < need:
        sl <<= 1
    return int(k), sl


def tile_pieces(c, K, tile=0):
    """pieces of a tile of a tile image: every run of result bytes -- header, gap, Task, tail, line feed; nothing fuses in these cases -- in
    pieces of 16"""
    n = 0
    for t in c.tx[tile * K:(tile + 1) * K]:
        cur = 0
        runs = [t["hlen"]]
        for code, sp, ln, sr in t["tasks"]:
            runs += [sr - cur, ln]
            cur = sr + ln
        runs += [c.res_len(t) - cur, 1 if t["hlen"] else 0]
        n += sum(-(-r // PIECE_BYTES) for r in runs)
    return n


def _slot_limit(over):
    """64 transcripts of 32 one-byte copies that fuse with nothing: 2048 pieces in the forced tile of 64 -- every slot the statistics give a
    tile (they would pick a smaller K); one '.' more is one piece more"""
    c = Case(seed=2250 + over)
    for u in range(65):
        c.open(off=13 * u, ref_len=500)
        c.fillers(32, ln=1)
        if over and u == 63:
            c.tail(1)
    k_rule, slots = tile_slots_for(c)
    assert slots == TILE_SLOTS_MAX and k_rule < 64 and tile_pieces(c, 64) == slots + over and sum(c.arena_len(t) for t in c.tx[:64]) < TILE_SPAN_MAX
    return _done(c, 64, (9,), pieces=(slots + over, slots), refused={9: ERR_UNSUPPORTED} if over else {})


case("tile_image", "a_tile_whose_pieces_fill_every_slot")(lambda: _slot_limit(0))
case("tile_image", "a_tile_with_one_piece_more_than_its_slots_is_refused")(lambda: _slot_limit(1))


# ================================================================== errors, by index
OFFENDERS = {
    "bad_code": (ERR_BAD_CODE, lambda c: c.raw(2, 0, 1, c.t["cur"])),
    "result_out_of_bounds": (ERR_RES_OOB, lambda c: c.raw(0, 5, 9, 1 << 20, advance=False)),
    "source_out_of_bounds": (ERR_SRC_OOB, lambda c: c.raw(0, 1 << 20, 3, c.t["cur"])),
    "not_contiguous": (ERR_NOT_CONTIGUOUS, lambda c: c.raw(0, 5, 3, c.t["cur"] - 1)),
}


def _error(rule, j, n_items=140):
    """the offender is item j of a one-transcript tile"""
    code, put = OFFENDERS[rule]
    c = Case(seed=2300 + j)
    c.open()
    c.fillers(j)
    g = put(c)
    c.fillers(n_items - j - 1)
    assert c.item_of(g, 1) == (0, j, n_items)
    c.reach = dict(at={k: emitted_at(j, n_items, k) for k in (6, 7)})
    return _done(c, 1, (6, 7), error=(code, g))


# items 1, 2 (and 3 for the dense parse) are context lanes of no window; 58 .. 63 are the first window's last emitted lanes and the second
# window's context and first emitted lanes (wave: the second window starts at item 60 and emits from 62; dense: at 58, from 62)
for _rule in OFFENDERS:
    for _j in (1, 2, 57, 58, 59, 60, 61, 62, 63, 64, 119, 121, 122):
        case("errors", f"{_rule}_at_item_{_j:03d}")(lambda r=_rule, j=_j: _error(r, j))


@case("errors")
def two_offenders_in_different_tiles_the_smaller_row_is_reported():
    c = Case(seed=2400)
    for u in range(6):
        c.open(off=u, ref_len=500)
        c.fillers(4)
        if u == 2:
            g = c.raw(0, 5, 3, c.t["cur"] - 1)
        if u == 4:
            c.raw(3, 0, 1, c.t["cur"])
        c.fillers(2)
    return _done(c, [1, 2], (6, 7), error=(ERR_NOT_CONTIGUOUS, g))


@case("errors")
def a_transcript_outside_the_resident_proteome():
    c = Case(prot_len=4096, seed=2401)
    c.open(off=0, ref_len=300)
    c.fillers(3)
    c.open(off=4000, ref_len=97)                         # 4000 + 97 > 4096
    g = c.fillers(2)[0]
    c.open(off=0, ref_len=300)
    c.fillers(3)
    assert c.tx[1]["off"] + c.tx[1]["ref_len"] == len(c.prot) + 1
    return _done(c, [1, 64], (6, 7), error=(ERR_SRC_OOB, g))


@case("errors")
def a_triple_broken_by_a_bad_task():
    c = Case(seed=2402)
    c.open()
    sp = c.take(40)
    c.ref(sp, 5)
    g = c.raw(1, 7, 1, c.t["cur"])                       # the literal reads past the transcript's (empty) alt tape
    c.ref(sp + 6, 5)
    return _done(c, 1, (6, 7), error=(ERR_SRC_OOB, g))


def good_stream():
    """what every batch must still build and execute after a refusal"""
    c = Case(seed=2500)
    c.open()
    c.fillers(3)
    c.triple(4, ord("o"), 5)
    c.tail(2)
    return _done(c, 1, (6, 7))


def expected_paths(c, K, kernel, desc, chunks):
    """What the build info must say, from the HOST image of the stream (descriptors in arena order, chunk table) and the tile size:
    two_pass        a tile holds more descriptors than its ROWS_TILE_SLOTS of the padded array
    cut_emit_pass   a 640-row segment holds more chunks than its slots of the cutter's padded table
    fell_back       the one call builds in one piece: either of the two, or -- a padded wave image, built for streams of at most
                    PAD_BYTES_PER_TASK_MAX result bytes per Task -- a chunk whose descriptors reach a third tile"""
    from stitch_rule import desc_len
    n_tiles = max(1, -(-len(c.tx) // K))
    base = np.cumsum([0] + [sum(c.arena_len(t) for t in c.tx[i * K:(i + 1) * K]) for i in range(n_tiles)])
    start = np.cumsum([0] + [desc_len(int(d)) for d in desc])[:-1]
    tile_of = np.searchsorted(base[1:], start, side="right")           # (a descriptor belongs to the tile its first byte lies in)
    two_pass = bool(len(desc)) and int(np.bincount(tile_of, minlength=n_tiles).max()) > ROWS_TILE_SLOTS
    out_bytes, n_tasks = int(base[-1]), c.n_tasks()
    pad = chunk_pad_for(out_bytes, n_tasks + (2 * len(c.tx) if c.fasta else 0), kernel)
    cut = False
    three = False
    if len(chunks):
        dst = (chunks[:, 1] & np.uint64((1 << 48) - 1)).astype(np.int64)
        cut = int(np.bincount(dst // (ROWS_SEG * ROW_BYTES)).max()) > pad
        if kernel == 6 and out_bytes <= PAD_BYTES_PER_TASK_MAX * n_tasks:
            first = (chunks[:, 0] & np.uint64((1 << 42) - 1)).astype(np.int64)
            n = ((chunks[:, 1] >> np.uint64(48)) & np.uint64(0x7FF)).astype(np.int64)
            three = bool(np.any(tile_of[first + n - 1] - tile_of[first] >= 2))
    return dict(two_pass=two_pass, cut_emit_pass=cut, fell_back=two_pass or cut or three)


def build(name):
    return CASES[name][1]()


def expand():
    """[(name, kernel, K)] of every build the GPU suite runs"""
    out = []
    for name in CASES:
        c = build(name)
        for kernel in c.kernels:
            for K in c.K:
                out.append((name, kernel, K))
    return out
