"""What the Python call layer (torrent_amd/verify.py, v2.py, hybrid.py) asks of the library, call by call, on the CPU:
every bulk call runs against a recording stand-in for _native.Context and its trace must equal the recorded one in
tests/golden/call_traces.json.  A trace entry is a library call with its arguments and the OPTIONS IN EFFECT at that
moment, so option writes may be reordered or merged, and nothing else may change.  The golden file is written by
running this file as a program (`python -m tests.test_call_trace`) at the commit whose behaviour is to be kept; the
one committed was recorded at 07a4297, the commit before the call layer's helpers were shared.

Also here: the option a cached context must not leak from one call into the next (TV_OPT_FILE_DIRECT_MIN), on the
stand-in and, marked gpu, on the library."""
import contextlib
import ctypes
import hashlib
import json
import os

import pytest

from tests import hybrid_util as hu
from tests import synth, v2_util
from torrent_amd import (_cpu, _native, hash_files, hash_files_hybrid, hash_files_v2, hash_pieces, hybrid,
                         make_torrent_hybrid, make_torrent_v2, merkle_v2, parse_metainfo_hybrid, parse_metainfo_v2, v2,
                         verify, verify_files, verify_files_hybrid, verify_files_v2, verify_payload,
                         verify_payload_hybrid, verify_payload_v2, verify_piece, verify_piece_v2, verify_pieces,
                         verify_stream, verify_stream_v2)
from torrent_amd.metainfo import FileInfo, make_info

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_traces.json")
L = 32 << 10
LENGTHS = [1, L, 17, 0, 2 * L + 5, 16385, 3 * L]            # (the list of tests/test_hybrid_host.py)
FILES = [bytes(synth.fill(40 + k, 0, n)) for k, n in enumerate(LENGTHS)]
PATHS = v2_util.file_names(len(FILES))
LINEAR = b"".join(FILES)
L1 = 1000                                                   # v1 pieces: a short last piece, files straddle pieces
DIR = os.path.join("no_such_dir", "call_trace")             # relative, so that no path depends on where the tests run
DIRECT_MIN_DEFAULT = 32 << 20                               # tv_ctx.h file_direct_min

OPT_NAMES = {getattr(_native, n): n[7:] for n in dir(_native) if n.startswith("TV_OPT_")}
# the library's defaults (tv_ctx.h)
DEFAULTS = {"RESIDENT": 1, "RESIDENT_BUDGET": 0, "STREAM_CHUNK": 0, "STREAM_ROWS": 0, "OPEN_RW": 1,
            "FILE_DIRECT_MIN": DIRECT_MIN_DEFAULT, "FILE_THREADS": 16, "LIST_SLOTS": 0}


def _ones(count: int) -> bytearray:
    bf = bytearray((count + 7) // 8)
    for j in range(count):
        bf[j >> 3] |= 0x80 >> (j & 7)
    return bf


class Recorder:
    """_native.Context stand-in: keeps the options, logs every other call with its arguments and the options in effect,
    and answers with made-up but fixed results.  A stream is one request over the whole shard, into a real slot."""

    row_bytes = _native.Context.row_bytes

    def __init__(self, root: str = "", window_pieces: int = 0):
        self.options = dict(DEFAULTS)
        self.log = []
        self.thread_budget = 16
        self.root, self.window_pieces = root, window_pieces
        self.shard_first = self.shard_count = 0
        self._v2_stream_bytes = None

    def enc(self, v):
        if v is None or isinstance(v, (bool, int, str)):
            return v.replace(self.root, "<tree>") if self.root and isinstance(v, str) else v
        if isinstance(v, _native.StreamReq):
            return {"piece": v.piece, "rows": v.rows, "offset": v.offset, "width": v.width}
        if isinstance(v, (bytes, bytearray, memoryview, ctypes.Array)):
            b = bytes(v)
            return {"len": len(b), "sha1": hashlib.sha1(b).hexdigest()}
        if hasattr(v, "tolist"):
            return v.tolist()
        if isinstance(v, (list, tuple)):
            return [self.enc(x) for x in v]
        if isinstance(v, hybrid.HybridResult):
            return {"bitfield": self.enc(v.bitfield), "v1": self.enc(v.v1), "v2": self.enc(v.v2)}
        if isinstance(v, v2.FileHashV2):
            return {"path": v.path, "length": v.length, "pieces_root": self.enc(v.pieces_root),
                    "layer": self.enc(v.layer)}
        if isinstance(v, BaseException):
            return {"raises": type(v).__name__, "message": str(v)}
        raise TypeError(type(v))

    def _call(self, name: str, *args) -> None:
        self.log.append([name, self.enc(args), dict(self.options)])

    def _bits(self, avail=None) -> bytes:
        return bytes(_ones(self.shard_count) if avail is None else avail)

    def _digests(self, tag: bytes, h) -> bytes:
        shard = range(self.shard_first, self.shard_first + self.shard_count)
        return b"".join(h(tag + b"%d" % i).digest() for i in shard)

    # -- options, layout, staging
    def set_option(self, key, value):
        self.options[OPT_NAMES.get(key, str(key))] = value

    def get_option(self, key):
        return self.options[OPT_NAMES.get(key, str(key))]

    def counter(self, key):
        self._call("counter", key)
        return {_native.TV_COUNTER_WINDOW_PIECES: self.window_pieces, _native.TV_COUNTER_BUDGET: 12345}.get(key, 0)

    def set_layout(self, total, piece_length, n_pieces, first=0, count=None):
        self._call("set_layout", total, piece_length, n_pieces, first, count)
        self.total_length, self.piece_length, self.n_pieces = total, piece_length, n_pieces
        self.shard_first, self.shard_count = first, count

    def set_digests(self, raw):
        self._call("set_digests", raw)

    def v2_set_pieces(self, piece_bytes, tree_leaves, hashes=None):
        self._call("v2_set_pieces", piece_bytes, tree_leaves, hashes)

    def stage(self, offset, data):
        self._call("stage", offset, data)

    def stage_many(self, parts):
        self._call("stage_many", list(parts))

    def stage_files(self, paths, file_offsets, linear_offsets, lens):
        self._call("stage_files", paths, file_offsets, linear_offsets, lens)
        return [0] * len(paths)

    # -- verify and hash
    def verify(self, avail=None):
        self._call("verify", avail)
        return self._bits(avail)

    def verify_host(self, src, avail=None):
        self._call("verify_host", src, avail)
        return self._bits(avail)

    def v2_verify(self, avail=None):
        self._call("v2_verify", avail)
        return self._bits(avail)

    def hybrid_verify(self, avail=None):
        self._call("hybrid_verify", avail)
        v1, v2_ = bytearray(self._bits(avail)), bytearray(self._bits(avail))
        v1[0] &= 0x7F                   # three different bitfields, so that their order shows in the result
        v2_[-1] &= 0x3F
        return bytes(a & b for a, b in zip(v1, v2_)), bytes(v1), bytes(v2_)

    def hash(self):
        self._call("hash")
        return self._digests(b"v1:", hashlib.sha1)

    def v2_hash(self):
        self._call("v2_hash")
        return self._digests(b"v2:", hashlib.sha256)

    def hybrid_hash(self):
        self._call("hybrid_hash")
        return self._digests(b"v1:", hashlib.sha1), self._digests(b"v2:", hashlib.sha256)

    # -- streams
    def _open(self, v2_bytes):
        self._v2_stream_bytes, self._pending, self._bad = v2_bytes, True, set()

    def stream_begin(self, avail=None):
        self._call("stream_begin", avail)
        self._open(None)

    def v2_stream_begin(self, piece_bytes, tree_leaves, hashes, avail=None):
        self._call("v2_stream_begin", piece_bytes, tree_leaves, hashes, avail)
        self._open(list(piece_bytes))

    def stream_next(self):
        self._call("stream_next")
        req = _native.StreamReq()
        if self._pending:
            self._pending = False
            self._slot = ctypes.create_string_buffer(self.shard_count * self.piece_length)
            req.piece, req.rows, req.offset, req.width = self.shard_first, self.shard_count, 0, self.piece_length
            req.slot, req.seq = ctypes.addressof(self._slot), 1
        return req

    def stream_unreadable(self, piece):
        self._call("stream_unreadable", piece)
        self._bad.add(piece)

    def stream_commit(self, req):
        self._call("stream_commit", req, self._slot)

    def stream_end(self):
        self._call("stream_end")
        bf = _ones(self.shard_count)
        for i in self._bad:
            j = i - self.shard_first
            bf[j >> 3] &= ~(0x80 >> (j & 7)) & 0xFF
        return bytes(bf)

    def stream_abort(self):
        self._call("stream_abort")

    def stream_file_table(self, lengths, paths, avail=None):
        self._call("stream_file_table", lengths, paths, avail)
        return self._bits(avail), [0] * len(paths)

    def v2_stream_file_table(self, piece_bytes, tree_leaves, hashes, lengths, paths, avail=None):
        self._call("v2_stream_file_table", piece_bytes, tree_leaves, hashes, lengths, paths, avail)
        return self._bits(avail), [0] * len(paths)


class _HostBuffer:
    """_native.PinnedBuffer stand-in: ordinary memory."""

    def __init__(self, nbytes: int):
        self._c = ctypes.create_string_buffer(max(1, nbytes))
        self.ptr, self.nbytes = ctypes.addressof(self._c), nbytes
        self.mv = memoryview(self._c).cast("B")[:nbytes]

    def close(self):
        pass


@contextlib.contextmanager
def stand_ins(contexts: dict, **ctx_args):
    """The call layer on recording contexts ({(device, slot): Recorder}, filled on first use), with a fixed CPU share."""
    @contextlib.contextmanager
    def fake_context(device, slot=0):
        yield contexts.setdefault((device, slot), Recorder(**ctx_args))

    patches = [(m, "_context", fake_context) for m in (verify, v2, hybrid, merkle_v2) if hasattr(m, "_context")]
    patches += [(verify, "_node_of", {0: 0}), (_cpu, "cpu_share", lambda: {"cores": 16}),
                (_cpu, "node_cpus", lambda node: 128), (_native, "PinnedBuffer", _HostBuffer)]
    saved = [(m, name, getattr(m, name)) for m, name, _ in patches]
    try:
        for m, name, new in patches:
            setattr(m, name, new)
        yield
    finally:
        for m, name, old in saved:
            setattr(m, name, old)


def record(fn, **ctx_args) -> dict:
    """One traced call on fresh contexts: what each context was asked, the result (or the exception) and the options
    each context is left with."""
    contexts: dict = {}
    with stand_ins(contexts, **ctx_args):
        try:
            result = fn()
        except Exception as e:          # noqa: BLE001  (the exception is part of the trace)
            result = e
    enc = Recorder(**ctx_args).enc
    keys = sorted(contexts)
    return {"contexts": {"%d/%d" % k: contexts[k].log for k in keys}, "result": enc(result),
            "left": {"%d/%d" % k: contexts[k].options for k in keys}}


class _Linear:
    """A Storage's get over LINEAR."""

    def get(self, offset: int, n: int):
        return LINEAR[offset:offset + n] if offset + n <= len(LINEAR) else None


def _v1_info():
    pieces = b"".join(hashlib.sha1(LINEAR[o:o + L1]).digest() for o in range(0, len(LINEAR), L1))
    return make_info(L1, pieces, "t", files=[FileInfo(n, list(p)) for n, p in zip(LENGTHS, PATHS)])


def _write_tree(root: str) -> None:
    for comps, d in zip(PATHS, FILES):
        p = os.path.join(root, *comps)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(d)


def trace_all(tree: str) -> dict:
    """{call name: trace} of every traced call, over one and two shards.  tree: an empty directory to write into."""
    _write_tree(tree)
    info = _v1_info()
    meta = parse_metainfo_v2(v2_util.torrent_v2(FILES, L, paths=PATHS))
    hmeta = parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS))
    assert meta is not None and hmeta is not None and info.n_pieces == 214
    holed = [None if k == 4 else d for k, d in enumerate(FILES)]

    def read(offset, n):
        return LINEAR[offset:offset + n]

    def read_to(offset, n):                         # None past an offset
        return None if offset + n > 150_000 else LINEAR[offset:offset + n]

    def read_raises(offset, n):
        if offset + n > 150_000:
            raise OSError("the disk went away")
        return LINEAR[offset:offset + n]

    def read_v2(k, offset, n):
        return FILES[k][offset:offset + n]

    out = {}
    for devices in ([0], [0, 0]):
        d = {"devices": devices}
        calls = {
            "verify_pieces": lambda: verify_pieces(info, _Linear(), **d),
            "verify_payload": lambda: verify_payload(info, LINEAR, **d),
            "verify_payload resident=False": lambda: verify_payload(info, LINEAR, resident=False, **d),
            "verify_payload over budget": lambda: verify_payload(info, LINEAR, budget=100_000, **d),
            "verify_stream": lambda: verify_stream(info, read, **d),
            "verify_stream chunk=4096": lambda: verify_stream(info, read, chunk=4096, **d),
            "verify_stream read None": lambda: verify_stream(info, read_to, **d),
            "verify_stream read raises": lambda: verify_stream(info, read_raises, chunk=4096, **d),
            "verify_files": lambda: verify_files(info, DIR, **d),
            "verify_files stream=True": lambda: verify_files(info, DIR, stream=True, **d),
            "verify_files direct_min=0": lambda: verify_files(info, DIR, direct_min=0, **d),
            "hash_files": lambda: hash_files(info, DIR, **d),
            "hash_pieces": lambda: hash_pieces(LINEAR, L1, **d),
            "verify_payload_v2": lambda: verify_payload_v2(meta, holed, **d),
            "verify_payload_v2 stream=True": lambda: verify_payload_v2(meta, holed, stream=True, **d),
            "verify_stream_v2": lambda: verify_stream_v2(meta, read_v2, **d),
            "verify_stream_v2 chunk=16384": lambda: verify_stream_v2(meta, read_v2, chunk=16384, **d),
            "verify_files_v2": lambda: verify_files_v2(meta, DIR, **d),
            "verify_files_v2 stream=True": lambda: verify_files_v2(meta, DIR, stream=True, **d),
            "hash_files_v2": lambda: hash_files_v2(tree, L, **d),
            "hash_files_hybrid": lambda: hash_files_hybrid(tree, L, **d),
            "make_torrent_v2": lambda: make_torrent_v2(tree, "http://example.com/announce", comment="c",
                                                       creation_date=1, piece_length=L, **d),
            "make_torrent_hybrid": lambda: make_torrent_hybrid(tree, "http://example.com/announce", comment="c",
                                                               creation_date=1, piece_length=L, **d),
            "verify_payload_hybrid": lambda: verify_payload_hybrid(hmeta, holed, **d),
            "verify_files_hybrid": lambda: verify_files_hybrid(hmeta, DIR, **d),
        }
        for name, fn in calls.items():
            out["%s, %d shard(s)" % (name, len(devices))] = record(fn, root=tree)
        # a layout the library could only hold in windows: the resident v2 and hybrid calls refuse it
        out["verify_files_v2 windowed, %d shard(s)" % len(devices)] = record(
            lambda: verify_files_v2(meta, DIR, budget=1 << 20, **d), root=tree, window_pieces=5)
        out["verify_files_hybrid windowed, %d shard(s)" % len(devices)] = record(
            lambda: verify_files_hybrid(hmeta, DIR, budget=1 << 20, **d), root=tree, window_pieces=5)
    out["verify_piece"] = record(lambda: verify_piece(info, 3, LINEAR[3 * L1:4 * L1]))
    out["verify_piece last"] = record(lambda: verify_piece(info, 213, LINEAR[213 * L1:]))
    out["verify_piece_v2"] = record(lambda: verify_piece_v2(meta, 4, FILES[4][L:2 * L]))
    return out


def test_call_traces_are_the_recorded_ones(tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(trace_all(str(tmp_path / "tree"))))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["contexts"].keys() == want[name]["contexts"].keys(), name
        for key, log in want[name]["contexts"].items():
            for k, (a, b) in enumerate(zip(got[name]["contexts"][key], log)):
                assert a == b, (name, key, k)
            assert len(got[name]["contexts"][key]) == len(log), (name, key)
        assert got[name]["result"] == want[name]["result"], name
        assert got[name]["left"] == want[name]["left"], name


def test_hybrid_calls_take_more_devices_than_there_are_shards(tmp_path):
    """10 pieces on three devices are shards of 8, 2 and 0 pieces: the empty one is empty in each of a hybrid call's
    results (it used to be indexed as if it held hybrid_verify's three)."""
    tree = str(tmp_path / "tree")
    _write_tree(tree)
    hmeta = parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS))
    contexts: dict = {}
    with stand_ins(contexts):
        got = verify_files_hybrid(hmeta, DIR, devices=[0, 0, 0])
        pieces, hashed = hash_files_hybrid(tree, L, devices=[0, 0, 0])
    assert sorted(contexts) == [(0, 0), (0, 1)]
    # (the stand-in clears the first bit of each shard's v1 bits and the first two of its last byte's v2 bits)
    assert (bytes(got.bitfield), bytes(got.v1), bytes(got.v2)) == (b"\x3f\x00", b"\x7f\x40", b"\x3f\x00")
    assert len(pieces) == 20 * 10 and [h.length for h in hashed] == LENGTHS


def _later_calls(tree: str) -> dict:
    meta = parse_metainfo_v2(v2_util.torrent_v2(FILES, L, paths=PATHS))
    hmeta = parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS))
    return {"verify_files_v2": lambda: verify_files_v2(meta, tree),
            "verify_files_hybrid": lambda: verify_files_hybrid(hmeta, tree),
            "hash_files_v2": lambda: hash_files_v2(tree, L), "hash_files_hybrid": lambda: hash_files_hybrid(tree, L)}


def test_a_direct_min_does_not_leak_into_the_next_call(tmp_path):
    """Contexts are cached, so a call must set every option it depends on: after verify_files(direct_min=0), the v2 and
    hybrid file calls on the same contexts stage with the default threshold, not with the leftover 0."""
    tree = str(tmp_path / "tree")
    _write_tree(tree)
    info = _v1_info()
    contexts: dict = {}
    with stand_ins(contexts):
        for name, later in _later_calls(tree).items():
            verify_files(info, tree, direct_min=0)
            ctx = contexts[(0, 0)]
            assert ctx.log[-2][0] == "stage_files" and ctx.log[-2][2]["FILE_DIRECT_MIN"] == 0
            del ctx.log[:]
            later()
            staged = [e for e in ctx.log if e[0] == "stage_files"]
            assert len(staged) == 1 and staged[0][2]["FILE_DIRECT_MIN"] == DIRECT_MIN_DEFAULT, name


@pytest.mark.gpu
def test_gpu_a_direct_min_does_not_leak_into_the_next_call(tmp_path, native):
    tree = str(tmp_path / "tree")
    _write_tree(tree)
    info = _v1_info()
    later = _later_calls(tree)
    for name in ("verify_files_v2", "verify_files_hybrid"):
        assert verify_files(info, tree, direct_min=0) == _ones(info.n_pieces)
        with verify._context(0) as ctx:
            assert ctx.get_option(native.TV_OPT_FILE_DIRECT_MIN) == 0
        got = later[name]()
        bits = [got] if name == "verify_files_v2" else [got.bitfield, got.v1, got.v2]
        assert all(b == _ones(10) for b in bits), name
        with verify._context(0) as ctx:
            assert ctx.get_option(native.TV_OPT_FILE_DIRECT_MIN) == DIRECT_MIN_DEFAULT, name


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        traces = trace_all(os.path.join(tmp, "tree"))
    with open(GOLDEN, "w") as f:
        json.dump(traces, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(traces)} traces -> {GOLDEN}")
