"""Shared by tests/test_stream_tables_ref.py (CPU) and tests/test_gpu_stream_tables.py: the layouts that drive the host
side of the stream engine (torrent_amd/csrc/tv_stream.hip) down the paths no smaller layout reaches -- file tables of
more than FdCache's 256 kept descriptors, units of more than one request, cold shards under small requests -- and their
expected results from references only:

  v1      Storage(fs_storage).get + hashlib.sha1 over a copy of the tree (fsStorage.get creates what is missing)
  v2      tests/v2_ref.py with have=
  hybrid  tests/hybrid_util.Layout.verdicts plus the header's readability rule: a piece is unreadable iff its file is
          missing, unopenable, or shorter than the piece's offset plus piece_bytes

and the geometry of tv_plan.h restated (stream_geometry and the row window here; v2_stream_geometry in
tests/test_gpu_v2_stream.py; hybrid_stream_geometry in tests/hybrid_stream_util.py).  Nothing here calls the library.
"""
from __future__ import annotations

import functools
import hashlib
import os

from tests import hybrid_stream_util as hsu
from tests import hybrid_util as hu
from tests import synth, v2_ref

K, M, G = 1 << 10, 1 << 20, 1 << 30
LEAF = 16 * K
SLOT = 64 * M                 # one ring slot: the rows of a request hold at most this
CACHED_FDS = 256              # tv_stream.hip FdCache::kCachedFds: descriptors a file-table call keeps open
TV_OK, TV_ERR_IO = 0, -5


def rnd(seed: int, n: int) -> bytes:
    return bytes(synth.fill(seed, 0, n))


def names(n: int) -> list:
    """Path components of n files whose sorted order is the list order (the file tree's), 16 files per directory."""
    return [["d%03d" % (k // 16), "f%04d.bin" % k] for k in range(n)]


def split(payload: bytes, sizes) -> list:
    out, o = [], 0
    for n in sizes:
        out.append(payload[o:o + n])
        o += n
    assert o == len(payload)
    return out


# ---- what differs on disk from what the torrent states ---------------------------------------------------------------

class Faults:
    """File indices per failing kind, and flipped bytes [(file, position)].  missing: not written; short: written
    without its last byte (cut: [(file, bytes)] written without that many); directory: a directory stands at its path;
    readonly: written, then chmod 0444 (unopenable where files are opened read + write, TV_OPT_OPEN_RW = 1, unless
    this process may write it anyway)."""
    KINDS = ("missing", "short", "directory", "readonly")

    def __init__(self, missing=(), short=(), directory=(), readonly=(), flips=(), cut=()):
        self.missing, self.short, self.directory, self.readonly = map(tuple, (missing, short, directory, readonly))
        self.flips, self.cut = tuple(flips), tuple(cut)

    def kind(self, name: str) -> tuple:
        return getattr(self, name)

    def failing(self, blocked: bool = True) -> set:
        """The files that cannot supply all of their bytes (blocked: a read-only file cannot be opened)."""
        return (set(self.missing) | set(self.short) | set(self.directory) | {k for k, _ in self.cut}
                | (set(self.readonly) if blocked else set()))

    def disk(self, files, blocked: bool) -> list:
        """What each file supplies: its bytes as written (flips applied, a short file without its last byte), or None
        (missing, a directory, or read-only and blocked)."""
        out = [bytearray(f) for f in files]
        for k, pos in self.flips:
            out[k][pos] ^= 0x20
        out = [bytes(b) for b in out]
        for k, n in tuple((k, 1) for k in self.short) + self.cut:
            out[k] = out[k][:-n]
        for k in self.missing + self.directory + (self.readonly if blocked else ()):
            out[k] = None
        return out


def write_tree(root: str, paths, files, faults: Faults, chmod: bool = True) -> list:
    """The tree as `faults` leaves it on disk -> the full path of every file."""
    disk = faults.disk(files, blocked=False)
    full = []
    for k, comps in enumerate(paths):
        p = os.path.join(root, *comps)
        full.append(p)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if k in faults.missing:
            continue
        if k in faults.directory:
            os.mkdir(p)
            continue
        with open(p, "wb") as f:
            f.write(disk[k])
    if chmod:
        make_readonly(full, faults)
    return full


def make_readonly(full, faults: Faults) -> None:
    for k in faults.readonly:
        os.chmod(full[k], 0o444)


def blocked_here(full, faults: Faults) -> bool:
    """Whether this process is refused a read + write open of the read-only files (root is not)."""
    return not all(os.access(full[k], os.W_OK) for k in faults.readonly)


def tree_listing(root: str) -> list:
    out = []
    for d, dirs, fs in os.walk(root):
        out += [os.path.join(d, x) for x in dirs + fs]
    return sorted(out)


def expected_status(lengths, faults: Faults, blocked: bool) -> list:
    """TV_ERR_IO for every file that holds bytes and whose open or read fails, else TV_OK.  (Holds for a layout where
    every failing file is reached: no two of them in one row, see V1Table.check / Aligned.check.)"""
    bad = faults.failing(blocked)
    return [TV_ERR_IO if k in bad and n else TV_OK for k, n in enumerate(lengths)]


def opens(faults: Faults, k: int, blocked: bool, open_rw: bool) -> bool:
    """Whether the library's open of file k succeeds: not a missing file, not a read-only one it may not write; a
    directory opens read-only (its reads fail), not read + write."""
    return not (k in faults.missing or (k in faults.readonly and blocked) or (k in faults.directory and open_rw))


def both_sides(faults: Faults, n_files: int) -> bool:
    """At least one file of each failing kind (and a flipped byte) on each side of position CACHED_FDS."""
    groups = [faults.kind(k) for k in Faults.KINDS] + [tuple(f for f, _ in faults.flips)]
    return all(any(k < CACHED_FDS for k in g) and any(CACHED_FDS <= k < n_files for k in g) for g in groups)


# ---- C1: many files, v1 ---------------------------------------------------------------------------------------------------

V1_L = 16 * K
_HEAD, _RUN, _RUNS, _TINY = 4, 47, 7, 40


def _run_base(r: int) -> int:
    return _HEAD + _RUN * r


def v1_tiny(r: int, t: int) -> int:
    return _run_base(r) + 1 + t


def v1_big(r: int) -> int:
    return _run_base(r) + _TINY + 2


def v1_mid(r: int) -> int:
    return v1_big(r) + 1


def v1_sizes() -> list:
    """336 files, ~100 pieces of 16 KiB: seven runs of [0, 40 tiny files (one piece spans >= 20 of them), 0, a file of
    eleven pieces, a mid-size one, 1 byte, one piece's worth (never aligned), 0] between zero-length files, files of
    several pieces before and after, and a short last piece."""
    L = V1_L
    ns = [0, 3 * L + 100, 0, 2 * L + 7]
    for r in range(_RUNS):
        ns += [0] + [250 + 13 * ((r * _TINY + t) % 8) for t in range(_TINY)] + [0, 11 * L - 77 + r, 9000 + 331 * r, 1, L, 0]
    return ns + [5 * L - 33, 0, 777]


class V1Table:
    """A v1 torrent: the files back to back, SHA-1 digests of the true bytes, and the faults on disk."""

    def __init__(self, L: int, sizes, seed: int, faults: Faults, files=None):
        self.L = L
        self.lengths = list(sizes)
        self.n = len(self.lengths)
        self.total = sum(self.lengths)
        self.P = -(-self.total // self.L)
        self.payload = rnd(seed, self.total) if files is None else b"".join(files)
        self.files = split(self.payload, self.lengths)
        self.start = [sum(self.lengths[:k]) for k in range(self.n)]
        self.paths = names(self.n)
        self.digests = b"".join(hashlib.sha1(self.payload[o:o + self.L]).digest() for o in range(0, self.total, self.L))
        self.faults = faults

    def piece_len(self, i: int) -> int:
        return min(self.L, self.total - i * self.L)

    def pieces_of(self, k: int) -> range:
        """The pieces file k has bytes in (empty for a zero-length file)."""
        if not self.lengths[k]:
            return range(0)
        return range(self.start[k] // self.L, (self.start[k] + self.lengths[k] - 1) // self.L + 1)

    def files_in_piece(self, i: int) -> list:
        """The files Storage.get's walk of piece i meets with bytes in it."""
        return [k for k in range(self.n) if i in self.pieces_of(k)]

    def check(self) -> None:
        """What expected_status relies on: no two failing files share a piece, none is empty, none ends at a piece
        boundary (its zero-length segment would decide the next piece too), and no flipped byte lies in one."""
        bad = sorted(self.faults.failing(True))
        seen = set()
        for k in bad:
            assert self.lengths[k] and (self.start[k] + self.lengths[k]) % self.L, k
            assert not seen & set(self.pieces_of(k)), k
            seen |= set(self.pieces_of(k))
        assert not {f for f, _ in self.faults.flips} & set(bad)

    def opened(self, C: int, blocked: bool, open_rw: bool) -> set:
        """The files a stream in columns of C bytes opens: every row [piece, column) walks its files in order and ends
        at the first one that cannot supply its bytes (the reader loop of tv_stream.hip, restated).  All but 256 of
        them are opened and closed around each read."""
        disk = self.faults.disk(self.files, blocked)
        out = set()
        for i in range(self.P):
            for off in range(0, self.piece_len(i), C):
                lo, hi = i * self.L + off, i * self.L + min(self.piece_len(i), off + C)
                for k in self.files_in_piece(i):
                    a, b = max(lo, self.start[k]), min(hi, self.start[k] + self.lengths[k])
                    if b <= a:
                        continue
                    if opens(self.faults, k, blocked, open_rw):
                        out.add(k)
                    if disk[k] is None or len(disk[k]) < b - self.start[k]:
                        break
        return out

    def info(self):
        from torrent_amd import FileInfo, make_info
        return make_info(self.L, self.digests, "many", files=[FileInfo(n, list(p)) for n, p in zip(self.lengths, self.paths)],
                         length=self.total)

    def expected_from_tree(self, root: str) -> bytes:
        """Storage(fs_storage).get + hashlib.sha1 over the tree at `root` (a copy: the reference creates what is
        missing there)."""
        from torrent_amd import Storage
        from torrent_amd.storage import fs_storage
        st = Storage(fs_storage, self.info(), root)
        ok = []
        for i in range(self.P):
            b = st.get(i * self.L, self.piece_len(i))
            ok.append(b is not None and hashlib.sha1(b).digest() == self.digests[20 * i:20 * i + 20])
        return hu.pack(ok)

    def expected_model(self, blocked: bool) -> bytes:
        """The same bits without a disk: a piece is 1 iff every file of its walk supplies its bytes of the piece and
        they hash to the digest (the CPU test holds expected_from_tree to it)."""
        disk = self.faults.disk(self.files, blocked)
        ok = []
        for i in range(self.P):
            lo, hi = i * self.L, i * self.L + self.piece_len(i)
            buf = bytearray()
            for k in self.files_in_piece(i):
                a, b = max(lo, self.start[k]) - self.start[k], min(hi, self.start[k] + self.lengths[k]) - self.start[k]
                if disk[k] is None or len(disk[k]) < b:
                    buf = None
                    break
                buf += disk[k][a:b]
            ok.append(buf is not None and hashlib.sha1(buf).digest() == self.digests[20 * i:20 * i + 20])
        return hu.pack(ok)


@functools.lru_cache(maxsize=None)
def v1_table() -> V1Table:
    """C1: every failing kind and a flipped byte on both sides of position 256.  The missing and the shadowed files are
    the last of their run of tiny files: a row's walk ends at the first file that fails, and the files behind it in the
    row would never be opened."""
    L, n = V1_L, len(v1_sizes())
    faults = Faults(missing=(v1_tiny(1, 39), v1_tiny(6, 39)), short=(v1_mid(0), v1_mid(6)),
                    directory=(v1_tiny(2, 39), v1_tiny(5, 39)), readonly=(v1_big(3), v1_big(5) + 3),
                    flips=((v1_big(0), 5 * L + 3), (v1_tiny(4, 5), 0), (v1_tiny(5, 38), 1), (v1_big(6), 17), (n - 1, 776)))
    return V1Table(L, v1_sizes(), 7001, faults)


def v1_column(L: int, chunk: int) -> int:
    """tv_stream.hip stream_column under an explicit TV_OPT_STREAM_CHUNK."""
    return max(64, min(min(chunk // 64 * 64, -(-L // 64) * 64), SLOT))


def v1_budget_geometry(L: int, count: int, budget: int, min_win: int = 2048) -> tuple:
    """tv_plan.h stream_geometry restated: (column bytes, pieces per window) of tv_stream_file_table under a budget
    (a warm shard: windows of at least 2,048 pieces, so a shard below that is one window)."""
    half = min((budget or G) // 2, hsu.CHUNK_MAX)
    lpad = min(-(-L // 64) * 64, SLOT)
    w = min(count, min_win)
    per = (half - 256) // w if half > 256 and w else 0
    wid = per - 256 if per > 256 else 64
    C = max(64, min(wid // 4096 * 4096 if wid >= 4096 else wid // 64 * 64, lpad))
    if C == lpad and w < count and half > 256:
        w = min(count, max(w, (half - 256) // (C + 256) // 64 * 64))
    return C, w


def v1_row_window(L: int, count: int, budget: int) -> int:
    """tv_stream.hip stream_row_window restated: whole pieces per window under TV_OPT_STREAM_ROWS."""
    pitch = -(-L // 64) * 64 + 256
    nbytes = min(4 * G, budget // 2) if budget else 4 * G
    return min(max(64, nbytes // pitch // 64 * 64), count)


def v1_rows_budget(L: int, rows: int = 64) -> int:
    return 2 * rows * (-(-L // 64) * 64 + 256)


# ---- C2 / C5 / C6: aligned tables (v2 and hybrid) -----------------------------------------------------------------------------

def request_plan(first: int, count: int, C: int, wn: int, L: int, req_bytes: int = 0) -> list:
    """[(piece, rows, offset)] of every request of a v2 / hybrid stream, in order: window by window, column by column,
    at most max(1, min(req_bytes or one slot, one slot) // C) rows each (tv_stream.hip set_geometry)."""
    per = max(1, (min(req_bytes, SLOT) if req_bytes else SLOT) // C)
    out = []
    for j0 in range(0, count, wn):
        wc = min(wn, count - j0)
        for col in range(-(-L // C)):
            out += [(first + j0 + r0, min(per, wc - r0), col * C) for r0 in range(0, wc, per)]
    return out


def requests_per_unit(count: int, C: int, wn: int, req_bytes: int = 0) -> list:
    """Requests of each window's units."""
    per = max(1, (min(req_bytes, SLOT) if req_bytes else SLOT) // C)
    return [-(-min(wn, count - j0) // per) for j0 in range(0, count, wn)]


class Aligned:
    """Files that each start a piece, as a v2 torrent (lay(False)) and as a hybrid one with or without a trailing pad
    (lay(True) / lay(False)), and the faults on disk."""

    def __init__(self, L: int, sizes, seed: int, faults: Faults):
        self.L, self.lengths, self.faults = L, list(sizes), faults
        self.n = len(self.lengths)
        self.files = split(rnd(seed, sum(self.lengths)), self.lengths)
        self.paths = names(self.n)
        self._lay = {}

    def lay(self, trailing: bool = False) -> hu.Layout:
        if trailing not in self._lay:
            self._lay[trailing] = hu.Layout(self.files, self.L, trailing)
        return self._lay[trailing]

    @property
    def P(self) -> int:
        return self.lay().P

    def check(self) -> None:
        bad = self.faults.failing(True)
        assert all(self.lengths[k] for k in bad) and not {f for f, _ in self.faults.flips} & bad

    def opened(self, blocked: bool, open_rw: bool) -> set:
        """The files a file-table call opens: every one that holds bytes and can be opened."""
        return {k for k, n in enumerate(self.lengths) if n and opens(self.faults, k, blocked, open_rw)}

    def unreadable(self, blocked: bool) -> set:
        """The header's rule: the pieces whose file is missing, unopenable, or shorter than offset + piece_bytes."""
        disk = self.faults.disk(self.files, blocked)
        return {i for i, (f, o, b, w) in enumerate(self.lay().table) if disk[f] is None or len(disk[f]) < o + b}

    def staged(self) -> list:
        """Full-length buffers holding what the disk holds where it holds something (the resident calls' input, and
        Layout.verdicts'); the bytes the disk lacks are the true ones, their pieces are unreadable anyway."""
        disk = self.faults.disk(self.files, blocked=False)
        return [f if d is None else d + f[len(d):] for f, d in zip(self.files, disk)]

    def readable_bits(self, blocked: bool) -> bytes:
        gone = self.unreadable(blocked)
        return hu.pack([i not in gone for i in range(self.P)])

    def expected_v2(self, blocked: bool) -> bytes:
        lay = self.lay()
        return v2_ref.expected_bitfield(self.faults.disk(self.files, blocked), self.L, lay.hashes, have=self.lengths)

    def expected_hybrid(self, blocked: bool, trailing: bool, pieces=None) -> tuple:
        """(bitfield, v1, v2) against the v1 `pieces` string given (default: the layout's own)."""
        lay = self.lay(trailing)
        ok1, ok2, _, _ = lay.verdicts(self.staged(), pieces)
        gone = self.unreadable(blocked)
        ok1 = [ok and i not in gone for i, ok in enumerate(ok1)]
        ok2 = [ok and i not in gone for i, ok in enumerate(ok2)]
        return hu.pack([a and b for a, b in zip(ok1, ok2)]), hu.pack(ok1), hu.pack(ok2)


MANY_L = 32 * K


def many_sizes() -> list:
    L = MANY_L
    return [1, 55, 56, 16383, 16384, 16385, L - 1, L, L + 1, 2 * L + 5, 0] * 31


@functools.lru_cache(maxsize=None)
def many() -> Aligned:
    """C2: 341 files of every edge size (310 hold bytes, so some 50 are opened past the kept descriptors), 403 pieces of
    32 KiB; every failing kind on both sides of position 256."""
    L = MANY_L
    faults = Faults(missing=(20, 270), short=(40, 290), directory=(60, 283), readonly=(100, 300),
                    flips=((9, 2 * L + 4), (30, 0), (128, 16384), (262, L), (271, 16384), (306, L + 3)))
    return Aligned(L, many_sizes(), 7100, faults)


def v2_launches(count: int, C: int, wn: int, L: int) -> int:
    """A v2 stream's launches as tests/test_gpu_v2_stream.py counts them: per window a column launch per column, a
    level launch per doubling of the columns and the finish launch."""
    ncol = L // C
    return -(-count // wn) * (ncol + ncol.bit_length() - 1 + 1)


# ---- C5: tall units -------------------------------------------------------------------------------------------------------------

TALL_L, TALL_P = 32 * K, 4096 + 70


def tall_sizes() -> list:
    """4,166 pieces in ten files whose tails put short and empty rows (and, in a hybrid torrent, pad ranges) on both
    sides of row 4096: a row of 100 bytes at 4090, then rows 4091-4098 = 1, 16384, 16385, L, L, L - 5, 20000, 55
    bytes, a 16,383-byte tail at 4159 and a 1-byte last row."""
    L = TALL_L
    return [4090 * L + 100, 1, 16384, 16385, L, 2 * L - 5, 20000, 55, 60 * L + 16383, 5 * L + 1]


@functools.lru_cache(maxsize=None)
def tall() -> Aligned:
    """Flipped bytes in row 4095, row 4096, the last row, and the second column of row 4100."""
    L = TALL_L
    return Aligned(L, tall_sizes(), 7200, Faults(flips=((5, 10), (5, L + 7), (9, 5 * L), (8, L + 16384 + 5))))


TALL_FLIPPED = (4095, 4096, 4100, 4165)
TALL_WINDOW = 2048 + 64       # rows per window of the second shape: a slot's 2,048 whole pieces and 64 more


# ---- C6: cold shards, small requests --------------------------------------------------------------------------------------------------

COLD_L, COLD_C, COLD_REQ = M, 256 * K, M


def cold_sizes() -> list:
    """Three files of about 5 MiB with odd tails and one under 1 MiB (never opened O_DIRECT); the last one is short on
    disk."""
    return [5 * M + 4093, 700 * K + 13, 5 * M + 2, 5 * M + 12345]


COLD_CUT = 2 * M + 777        # bytes the last file lacks on disk: its tail pieces are unreadable


@functools.lru_cache(maxsize=None)
def cold() -> Aligned:
    L = COLD_L
    return Aligned(L, cold_sizes(), 7300, Faults(flips=((0, 3 * L + 5), (1, 700 * K), (2, 5 * M + 1)), cut=((3, COLD_CUT),)))


@functools.lru_cache(maxsize=None)
def cold_v1() -> V1Table:
    """The same files back to back, as a v1 torrent (file 1 starts at 5 MiB + 4093: rows through the aligned scratch)."""
    c = cold()
    return V1Table(COLD_L, c.lengths, 0, c.faults, files=c.files)
