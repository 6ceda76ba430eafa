"""Streamed creation on the CPU: the seven tv_*stream_hash* calls are declared by the header and bound by
torrent_amd/_native.py, the creation hosts take stream= (default False), and hash_stream / hash_stream_v2 /
hash_stream_hybrid drive begin, next, commit and stream_hash_end in that order on every shard -- against a stand-in for
_native.Context (the pattern of tests/test_hybrid_stream_host.py; its own copy) that hashes the rows it is given with
hashlib and tests/v2_ref.py, so the joined result is checked against the whole torrent's hashes."""
import contextlib
import ctypes
import hashlib
import inspect
import os
import re

import pytest

from tests import hybrid_util as hu
from tests import synth, v2_ref
from torrent_amd import (_cpu, _native, hash_files, hash_files_hybrid, hash_files_v2, hash_pieces, hash_stream,
                         hash_stream_hybrid, hash_stream_v2, make_torrent, make_torrent_hybrid, make_torrent_v2, verify)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tv_stream_hash_begin", "tv_v2_stream_hash_begin", "tv_hybrid_stream_hash_begin", "tv_stream_hash_end",
         "tv_stream_hash_file_table", "tv_v2_stream_hash_file_table", "tv_hybrid_stream_hash_file_table"]
OPT_NAMES = {getattr(_native, n): n[7:] for n in dir(_native) if n.startswith("TV_OPT_")}

L = 32 << 10
LENGTHS = [1, L, 17, 0, 2 * L + 5, 16385, 3 * L, 8 * L + 9]         # 19 pieces: two shards of 16 and 3
FILES = [bytes(synth.fill(80 + k, 0, n)) for k, n in enumerate(LENGTHS)]
LAY = hu.Layout(FILES, L)


def test_the_seven_calls_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "torrent_verify.h")).read()
    bound = {n for n, _, _ in _native.SYMBOLS}
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in bound, name
    for wrapper in ("stream_hash_begin", "v2_stream_hash_begin", "hybrid_stream_hash_begin", "stream_hash_end",
                    "stream_hash_file_table", "v2_stream_hash_file_table", "hybrid_stream_hash_file_table"):
        assert callable(getattr(_native.Context, wrapper))
    ts = open(os.path.join(ROOT, "ts", "verify.ts")).read()
    for name in NAMES:
        assert re.search(r"^\s*%s: \{" % name, ts, re.M), name


def test_the_stream_parameters_default_to_false():
    for fn in (hash_pieces, hash_files, hash_files_v2, make_torrent_v2, hash_files_hybrid, make_torrent_hybrid,
               make_torrent):
        assert inspect.signature(fn).parameters["stream"].default is False, fn.__name__


class Recorder:
    """_native.Context stand-in for a creation stream: one request over the whole shard into a real slot; stream_hash_end
    hashes the committed rows on the CPU."""

    row_bytes = _native.Context.row_bytes

    def __init__(self):
        self.options, self.log, self.thread_budget = {}, [], 16
        self.shard_first = self.shard_count = 0
        self._v2_stream_bytes = None

    def _call(self, name, *args):
        keys = ("RESIDENT", "RESIDENT_BUDGET", "STREAM_CHUNK", "STREAM_ROWS")
        self.log.append((name, args, tuple(self.options.get(k) for k in keys)))

    def set_option(self, key, value):
        self.options[OPT_NAMES.get(key, str(key))] = value

    def counter(self, key):
        return 0

    def set_layout(self, total, piece_length, n_pieces, first=0, count=None):
        self._call("set_layout", total, piece_length, n_pieces, first, count)
        self.total_length, self.piece_length, self.n_pieces = total, piece_length, n_pieces
        self.shard_first, self.shard_count = first, count

    def set_digests(self, raw):
        raise AssertionError("a creation stream needs no digests")

    def _begin(self, kind, pb=None, tl=None):
        self._kind, self._pending, self._tl = kind, True, None if tl is None else list(tl)
        self._v2_stream_bytes = None if pb is None else list(pb)

    def stream_hash_begin(self):
        self._call("stream_hash_begin")
        self._begin("v1")

    def v2_stream_hash_begin(self, piece_bytes, tree_leaves):
        self._call("v2_stream_hash_begin", list(piece_bytes), list(tree_leaves))
        self._begin("v2", piece_bytes, tree_leaves)

    def hybrid_stream_hash_begin(self, piece_bytes, tree_leaves):
        self._call("hybrid_stream_hash_begin", list(piece_bytes), list(tree_leaves))
        self._begin("hybrid", piece_bytes, tree_leaves)

    def stream_next(self):
        req = _native.StreamReq()
        if self._pending:
            self._pending = False
            self._slot = ctypes.create_string_buffer(b"\xaa" * (self.shard_count * self.piece_length))
            req.piece, req.rows, req.offset, req.width = self.shard_first, self.shard_count, 0, self.piece_length
            req.slot, req.seq = ctypes.addressof(self._slot), 1
            self._req = req
        self._call("stream_next", req.rows)
        return req

    def stream_unreadable(self, piece):
        raise AssertionError("a creation stream cannot skip a piece")

    def stream_commit(self, req):
        self._call("stream_commit")
        self._rows = bytes(self._slot)

    def stream_end(self):
        raise AssertionError("a creation host ends its stream with stream_hash_end")

    hybrid_stream_end = stream_end

    def stream_hash_end(self):
        self._call("stream_hash_end")
        Lp, d, r = self.piece_length, b"", b""
        for j in range(self.shard_count):
            i = self.shard_first + j
            n = self.row_bytes(self._req, j)
            row = self._rows[j * Lp:j * Lp + n]
            if self._kind != "v2":      # the piece's v1 bytes: its file bytes and, in a hybrid torrent, the pad's zeros
                d += hashlib.sha1(row + bytes(min(Lp, self.total_length - i * Lp) - n)).digest()
            if self._kind != "v1":
                r += v2_ref.piece_root(row, self._tl[i])
        return (d, r) if self._kind == "hybrid" else (d or r)

    def stream_abort(self):
        self._call("stream_abort")


@contextlib.contextmanager
def stand_ins(contexts):
    @contextlib.contextmanager
    def fake_context(device, slot=0):
        yield contexts.setdefault((device, slot), Recorder())

    patches = [(verify, "_context", fake_context), (verify, "_node_of", {0: 0}),
               (_cpu, "cpu_share", lambda: {"cores": 16}), (_cpu, "node_cpus", lambda node: 128)]
    saved = [(m, name, getattr(m, name)) for m, name, _ in patches]
    try:
        for m, name, new in patches:
            setattr(m, name, new)
        yield
    finally:
        for m, name, old in saved:
            setattr(m, name, old)


def _read(bufs):
    def read(k, offset, n):
        return None if bufs[k] is None else bufs[k][offset:offset + n]
    return read


STREAM = ["stream_next", "stream_commit", "stream_next", "stream_hash_end"]


def test_hash_stream_call_sequence_and_shards():
    P, last = 19, 777
    total = (P - 1) * L + last
    payload = bytes(synth.fill(5, 0, total))
    want = b"".join(hashlib.sha1(payload[i * L:(i + 1) * L]).digest() for i in range(P))
    contexts = {}
    with stand_ins(contexts):
        got = hash_stream(total, L, lambda off, n: payload[off:off + n], devices=[0, 0], threads=1)
    assert got == want
    for (first, count), key in (((0, 16), (0, 0)), ((16, 3), (0, 1))):
        log = contexts[key].log
        assert [e[0] for e in log] == ["set_layout", "stream_hash_begin"] + STREAM
        # no resident payload, no budget, whole pieces per row (the geometry of verify_stream)
        assert log[0][1] == (total, L, P, first, count) and log[0][2] == (0, 0, 0, 1)
        assert log[2][1] == (count,)
        assert contexts[key].options["STREAM_CHUNK"] == 0 and contexts[key].options["STREAM_ROWS"] == 0
        assert contexts[key].options["RESIDENT"] == 1                       # (on again once the layout is set)


def test_hash_stream_v2_call_sequence_and_shards():
    contexts = {}
    with stand_ins(contexts):
        got = hash_stream_v2(LENGTHS, L, _read(FILES), devices=[0, 0], chunk=16 << 10, threads=1, budget=1 << 27)
    assert got == b"".join(LAY.hashes)
    for (first, count), key in (((0, 16), (0, 0)), ((16, 3), (0, 1))):
        log = contexts[key].log
        assert [e[0] for e in log] == ["set_layout", "v2_stream_hash_begin"] + STREAM
        assert log[0][1] == (LAY.total, L, 19, first, count) and log[0][2] == (0, 1 << 27, 16 << 10, 0)
        assert log[1][1] == (LAY.pb, LAY.tl)                                # the GLOBAL table, on every shard


def test_hash_stream_hybrid_call_sequence_and_shards():
    contexts = {}
    with stand_ins(contexts):
        pieces, roots = hash_stream_hybrid(LENGTHS, L, _read(FILES), devices=[0, 0], threads=1)
    assert pieces == LAY.pieces and roots == b"".join(LAY.hashes)
    for (first, count), key in (((0, 16), (0, 0)), ((16, 3), (0, 1))):
        log = contexts[key].log
        assert [e[0] for e in log] == ["set_layout", "hybrid_stream_hash_begin"] + STREAM
        assert log[0][1] == (LAY.total, L, 19, first, count)                # the v1 space: no pad after the last file


@pytest.mark.parametrize("kind", ["v1", "v2", "hybrid"])
def test_a_short_read_raises_before_any_output(kind):
    bufs = list(FILES)
    bufs[4] = FILES[4][:L + 3]                                              # its second piece reads short
    contexts = {}
    with stand_ins(contexts), pytest.raises(FileNotFoundError, match="missing or shorter"):
        if kind == "v1":
            lin = b"".join(FILES)
            hash_stream(len(lin) + 1, L, lambda off, n: lin[off:off + n], threads=1)    # one byte short
        elif kind == "v2":
            hash_stream_v2(LENGTHS, L, _read(bufs), threads=1)
        else:
            hash_stream_hybrid(LENGTHS, L, _read(bufs), threads=1)
    names = [e[0] for e in contexts[(0, 0)].log]
    assert names[-1] == "stream_abort" and "stream_hash_end" not in names and "stream_commit" not in names


class TableRecorder(Recorder):
    """... whose file-table calls report file 1 as short (TV_ERR_IO: no hashes)."""

    def _table(self, name, *args):
        self._call(name, *args)
        self.open_rw = self.options.get("OPEN_RW")
        return None, [0, _native.TV_ERR_IO] + [0] * 8

    def stream_hash_file_table(self, lengths, paths):
        return self._table("stream_hash_file_table", list(lengths), list(paths))

    def v2_stream_hash_file_table(self, pb, tl, lengths, paths):
        return self._table("v2_stream_hash_file_table", list(pb), list(tl), list(lengths), list(paths))

    def hybrid_stream_hash_file_table(self, pb, tl, lengths, paths):
        return self._table("hybrid_stream_hash_file_table", list(pb), list(tl), list(lengths), list(paths))


@pytest.mark.parametrize("kind", ["v1", "v2", "hybrid"])
def test_stream_true_with_a_short_file_raises(kind, tmp_path, monkeypatch):
    from torrent_amd import FileInfo, make_info
    monkeypatch.setattr(verify, "_context", contextlib.contextmanager(lambda device, slot=0: (yield rec)))
    monkeypatch.setattr(verify, "_node_of", {0: 0})
    rec = TableRecorder()
    names = ["a", "b", "c"]
    sizes = [L + 1, 2 * L, 5]
    for n, s in zip(names, sizes):
        (tmp_path / n).write_bytes(bytes(s))
    files = [([n], s) for n, s in zip(names, sizes)]
    if kind == "v1":
        info = make_info(L, bytes(20 * 4), "t", files=[FileInfo(length=s, path=[n]) for n, s in zip(names, sizes)])
        with pytest.raises(FileNotFoundError, match="^hash_files: a file is missing or shorter than its declared length$"):
            hash_files(info, str(tmp_path), stream=True, budget=1 << 26)
        call = "stream_hash_file_table"
    elif kind == "v2":
        with pytest.raises(FileNotFoundError, match="^hash_files_v2: a file is missing or shorter"):
            hash_files_v2(str(tmp_path), L, files=files, stream=True, budget=1 << 26)
        call = "v2_stream_hash_file_table"
    else:
        with pytest.raises(FileNotFoundError, match="^hash_files_hybrid: a file is missing or shorter"):
            hash_files_hybrid(str(tmp_path), L, files=files, stream=True, budget=1 << 26)
        call = "hybrid_stream_hash_file_table"
    assert [e[0] for e in rec.log] == ["set_layout", call]
    assert rec.log[0][2][:2] == (0, 1 << 26)                  # no resident payload, the caller's budget
    assert rec.open_rw == 0 and rec.options["OPEN_RW"] == 1   # read-only while it runs, read + write again afterwards
