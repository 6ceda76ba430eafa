"""The stream hosts of torrent_amd/hybrid.py (verify_stream_hybrid, verify_payload_hybrid(stream=True),
verify_files_hybrid(stream=True)) on the CPU, against a recording stand-in for _native.Context (the pattern of
tests/test_call_trace.py's Recorder; its own copy): the call sequence each shard makes and the options in effect, the
sharding of `avail`, the HybridResult and its `disagree`, and that a None or short read clears exactly that piece in
all three bitfields."""
import contextlib
import ctypes

from tests import hybrid_util as hu
from tests import synth, v2_util
from torrent_amd import (_cpu, _native, parse_metainfo_hybrid, verify, verify_files_hybrid, verify_payload_hybrid,
                         verify_stream_hybrid)

L = 32 << 10
LENGTHS = [1, L, 17, 0, 2 * L + 5, 16385, 3 * L, 8 * L + 9]         # 19 pieces: two shards of 16 and 3
FILES = [bytes(synth.fill(60 + k, 0, n)) for k, n in enumerate(LENGTHS)]
PATHS = v2_util.file_names(len(FILES))
OPT_NAMES = {getattr(_native, n): n[7:] for n in dir(_native) if n.startswith("TV_OPT_")}
V1_BAD, V2_BAD = 2, 5                                               # global pieces the stand-in's kernels refuse


def _bits(first, count, clear=()):
    return hu.pack([first + j not in clear for j in range(count)])


class Recorder:
    """_native.Context stand-in: keeps the options, logs the calls with the options that matter to a stream, and
    answers a hybrid stream with v1 = all but V1_BAD, v2 = all but V2_BAD, less the unavailable and unreadable pieces.
    A stream is one request over the whole shard, into a real slot."""

    row_bytes = _native.Context.row_bytes

    def __init__(self):
        self.options, self.log, self.thread_budget = {}, [], 16
        self.shard_first = self.shard_count = 0
        self._v2_stream_bytes = None

    def _call(self, name, *args):
        keys = ("RESIDENT", "RESIDENT_BUDGET", "STREAM_CHUNK", "STREAM_ROWS", "OPEN_RW")
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
        self._call("set_digests", bytes(raw))

    def _answer(self):
        gone = {self.shard_first + j for j in range(self.shard_count)
                if self._avail is not None and not (self._avail[j >> 3] >> (7 - (j & 7))) & 1} | self._bad
        v1 = _bits(self.shard_first, self.shard_count, gone | {V1_BAD})
        v2 = _bits(self.shard_first, self.shard_count, gone | {V2_BAD})
        return bytes(a & b for a, b in zip(v1, v2)), v1, v2

    def hybrid_stream_begin(self, piece_bytes, tree_leaves, hashes, avail=None):
        self._call("hybrid_stream_begin", list(piece_bytes), list(tree_leaves), bytes(hashes),
                   None if avail is None else bytes(avail))
        self._v2_stream_bytes, self._pending, self._bad, self._avail = list(piece_bytes), True, set(), avail

    def stream_next(self):
        req = _native.StreamReq()
        if self._pending:
            self._pending = False
            self._slot = ctypes.create_string_buffer(self.shard_count * self.piece_length)
            req.piece, req.rows, req.offset, req.width = self.shard_first, self.shard_count, 0, self.piece_length
            req.slot, req.seq = ctypes.addressof(self._slot), 1
        self._call("stream_next", req.rows)
        return req

    def stream_unreadable(self, piece):
        self._bad.add(piece)

    def stream_commit(self, req):
        self._call("stream_commit", bytes(self._slot))

    def hybrid_stream_end(self):
        self._call("hybrid_stream_end")
        return self._answer()

    def stream_end(self):
        raise AssertionError("a hybrid host ends its stream with hybrid_stream_end")

    def stream_abort(self):
        self._call("stream_abort")

    def hybrid_stream_file_table(self, piece_bytes, tree_leaves, hashes, lengths, paths, avail=None):
        self._call("hybrid_stream_file_table", list(piece_bytes), list(tree_leaves), bytes(hashes), list(lengths),
                   [str(p) for p in paths], avail)
        self._bad, self._avail = set(), avail
        return self._answer(), [0] * len(paths)


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


def _meta():
    meta = parse_metainfo_hybrid(hu.torrent_hybrid(FILES, L, paths=PATHS))
    assert meta is not None and meta.n_pieces == 19
    return meta


def _read(bufs):
    def read(k, offset, n):
        return None if bufs[k] is None else bufs[k][offset:offset + n]
    return read


def _slot_image(meta, first, count, bufs, skip=()):
    """What the rows of the one request hold: every piece's file bytes at its row, zeros elsewhere."""
    lay = meta.layout
    img = bytearray(count * L)
    for j in range(count):
        i = first + j
        if i in skip:
            continue
        k, o, n = lay.piece_file[i], lay.piece_offset[i], lay.piece_bytes[i]
        img[j * L:j * L + n] = bufs[k][o:o + n]
    return bytes(img)


def test_verify_stream_hybrid_call_sequence_and_result():
    meta, lay = _meta(), _meta().layout
    contexts = {}
    avail = bytearray(_bits(0, 19, {9, 17}))
    with stand_ins(contexts):
        r = verify_stream_hybrid(meta, _read(FILES), devices=[0, 0], avail=bytes(avail), chunk=64 << 10, threads=1,
                                 budget=1 << 28)
    assert sorted(contexts) == [(0, 0), (0, 1)]
    hashes = bytes(lay.hashes)
    for (first, count), key in (((0, 16), (0, 0)), ((16, 3), (0, 1))):
        shard_avail = hu.pack([first + j not in (9, 17) for j in range(count)])
        on = (0, 1 << 28, 64 << 10, 0, None)                  # not resident, the budget, the chunk, rows off
        want = [("set_layout", (meta.total_length, L, 19, first, count), on),
                ("set_digests", (meta.pieces,), on),
                # (TV_OPT_RESIDENT is on again once the layout is set)
                ("hybrid_stream_begin", (list(lay.piece_bytes), list(lay.tree_leaves), hashes, shard_avail),
                 (1,) + on[1:]),
                ("stream_next", (count,), (1,) + on[1:]),
                ("stream_commit", (_slot_image(meta, first, count, FILES),), (1,) + on[1:]),
                ("stream_next", (0,), (1,) + on[1:]),
                ("hybrid_stream_end", (), (1,) + on[1:])]
        assert contexts[key].log == want
        assert contexts[key].options["STREAM_CHUNK"] == 0 and contexts[key].options["STREAM_ROWS"] == 0
    assert bytes(r.v1) == _bits(0, 19, {9, 17, V1_BAD}) and bytes(r.v2) == _bits(0, 19, {9, 17, V2_BAD})
    assert bytes(r.bitfield) == _bits(0, 19, {9, 17, V1_BAD, V2_BAD}) and r.disagree == [V1_BAD, V2_BAD]


def test_a_none_or_short_read_clears_exactly_that_piece():
    meta = _meta()
    lay = meta.layout
    bufs = list(FILES)
    bufs[2] = None                                            # the 17-byte file: piece 2
    bufs[7] = FILES[7][:4 * L + 100]                          # pieces 10 .. 13 whole, 14 .. 18 short or empty reads
    p7 = lay.file_offset[7] // L
    gone = {2} | set(range(p7 + 4, 19))
    contexts = {}
    with stand_ins(contexts):
        r = verify_payload_hybrid(meta, bufs, stream=True)
    assert bytes(r.v1) == _bits(0, 19, gone | {V1_BAD}) and bytes(r.v2) == _bits(0, 19, gone | {V2_BAD})
    assert bytes(r.bitfield) == _bits(0, 19, gone | {V1_BAD, V2_BAD}) and r.disagree == [V2_BAD]
    log = contexts[(0, 0)].log
    assert [e[0] for e in log] == ["set_layout", "set_digests", "hybrid_stream_begin", "stream_next", "stream_commit",
                                   "stream_next", "hybrid_stream_end"]
    assert log[0][1] == (meta.total_length, L, 19, 0, 19) and log[0][2][:2] == (0, 0)     # no budget: the default
    assert log[4][1] == (_slot_image(meta, 0, 19, FILES, skip=gone),)


def test_an_exception_in_read_aborts_the_stream():
    meta = _meta()
    contexts = {}

    def read(k, offset, n):
        raise OSError("disk")

    with stand_ins(contexts):
        try:
            verify_stream_hybrid(meta, read, threads=1)
            raise AssertionError("not raised")
        except OSError:
            pass
    assert [e[0] for e in contexts[(0, 0)].log][-2:] == ["stream_next", "stream_abort"]


def test_verify_files_hybrid_stream_call_sequence(tmp_path):
    meta = _meta()
    lay = meta.layout
    contexts = {}
    with stand_ins(contexts):
        r = verify_files_hybrid(meta, str(tmp_path), devices=[0, 0], threads=3, budget=1 << 27, stream=True)
    paths = [str(tmp_path.joinpath(*comps)) for comps in PATHS]
    for (first, count), key in (((0, 16), (0, 0)), ((16, 3), (0, 1))):
        log = contexts[key].log
        assert [e[0] for e in log] == ["set_layout", "set_digests", "hybrid_stream_file_table"]
        assert log[0][1] == (meta.total_length, L, 19, first, count) and log[0][2] == (0, 1 << 27, 0, 0, None)
        assert log[1][1] == (meta.pieces,)
        # read-only while the call runs (a verify writes nothing), read + write again afterwards
        assert log[2][1] == (list(lay.piece_bytes), list(lay.tree_leaves), bytes(lay.hashes), LENGTHS, paths, None)
        assert log[2][2] == (1, 1 << 27, 0, 0, 0) and contexts[key].options["OPEN_RW"] == 1
        assert contexts[key].options["FILE_THREADS"] == 3
    assert bytes(r.v1) == _bits(0, 19, {V1_BAD}) and bytes(r.v2) == _bits(0, 19, {V2_BAD})
    assert r.disagree == [V1_BAD, V2_BAD]


def test_the_resident_defaults_are_unchanged():
    """stream=False makes no stream call (tests/test_call_trace.py holds the whole trace to its golden file)."""
    import inspect
    for fn in (verify_payload_hybrid, verify_files_hybrid):
        assert inspect.signature(fn).parameters["stream"].default is False
