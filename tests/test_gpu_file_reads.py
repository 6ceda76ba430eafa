"""Which path every chunk of a file read takes (tv_files.hip's stage_units / stage_small, tv_stream.hip's row reader),
pinned by the phase clock (_reset_file_clock / _file_clock) next to the bitfield: the mapped page-cache window, the
buffered ring read, the O_DIRECT ring read, the bounce read, the refused O_DIRECT read's fallback, and the streamed rows.

The layout: 16 KiB pieces, TV_OPT_FILE_CHUNK = TV_OPT_FILE_DIRECT_MIN = 65,536, three long files of 200,003, 131,072 and
70,001 bytes and a 1,000-byte file after them (the small-segment path in the same call), a short last piece and one
corrupted piece per file.  File 1 starts at linear offset 200,003 and file 2 at 331,075: both are 3 mod 4, so only
file 0's file and linear offsets agree mod 4 (what can be mapped-direct or read O_DIRECT is worked out from the offsets
below, not written down).  TV_FILE_BYTES_READ counts the long segments' ring reads only (tv_options_internal.h), so the
byte sums are over the long files and the small file's read shows as time in the `small` phase.  Every call runs in a
context of its own, so no option outlives its case."""
import errno
import hashlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

L = 16384
SIZES = [200003, 131072, 70001, 1000]
TOTAL = sum(SIZES)
P = -(-TOTAL // L)
MIN = 65536
CORRUPT = (3, 15, 22, P - 1)          # a piece inside file 0, 1, 2, and the short last piece (file 2's tail + file 3)
STARTS = [sum(SIZES[:k]) for k in range(len(SIZES))]
LONG = sum(n for n in SIZES if n >= MIN)                                       # bytes staged by stage_units
AGREE = sum(n for o, n in zip(STARTS, SIZES) if n >= MIN and o % 4 == 0)       # (file offset 0) ^ linear == 0 mod 4
assert TOTAL % L and STARTS[1] % 4 == 3 and AGREE == SIZES[0]


def _bits(bf, n):
    return [(bf[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def _layout(oracle, tmp_path, cut=0):
    """The files on disk (file 2 shortened by `cut` bytes) -> (digests, paths, expected bits by Storage.get + hashlib)."""
    from torrent_amd import FileInfo, Storage, make_info
    from torrent_amd.storage import fs_storage
    payload = bytes(oracle.synth_fill(91, 0, TOTAL))
    digests = bytearray(b"".join(hashlib.sha1(payload[i * L:min(TOTAL, (i + 1) * L)]).digest() for i in range(P)))
    for i in CORRUPT:
        digests[20 * i + 2] ^= 0x10
    paths, files = [], []
    for k, (o, n) in enumerate(zip(STARTS, SIZES)):
        p = tmp_path / f"f{k}.bin"
        p.write_bytes(payload[o:o + n - (cut if k == 2 else 0)])
        paths.append(str(p))
        files.append(FileInfo(n, [f"f{k}.bin"]))
    info = make_info(L, bytes(digests), "reads", files=files, length=TOTAL)
    st = Storage(fs_storage, info, str(tmp_path))
    want = []
    for i in range(P):
        b = st.get(i * L, min(L, TOTAL - i * L))
        want.append(int(b is not None and hashlib.sha1(b).digest() == bytes(digests[20 * i:20 * i + 20])))
    return bytes(digests), paths, want


def _staged(native, digests, paths, before=None, **opts):
    """One tv_stage_file_table + tv_verify in a context of its own with the options set -> (bits, statuses, clock)."""
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_FILE_CHUNK, 65536)
        ctx.set_option(native.TV_OPT_FILE_DIRECT_MIN, MIN)
        for k, v in opts.items():
            ctx.set_option(getattr(native, "TV_OPT_" + k), v)
        ctx.set_layout(TOTAL, L, P)
        ctx.set_digests(digests)
        if before:
            before()
        ctx._reset_file_clock()
        status = ctx.stage_file_table(SIZES, paths)
        clock = ctx._file_clock()
        return _bits(ctx.verify(), P), status, clock


def _streamed(native, digests, paths, **opts):
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_RESIDENT, 0)
        for k, v in opts.items():
            ctx.set_option(getattr(native, "TV_OPT_" + k), v)
        ctx.set_layout(TOTAL, L, P)
        ctx.set_digests(digests)
        ctx._reset_file_clock()
        bits, status = ctx.stream_file_table(SIZES, paths)
        return _bits(bits, P), status, ctx._file_clock()


def test_warm_direct_windows(native, oracle, tmp_path):
    """TV_OPT_FILE_DIRECT = 1: 64 KiB windows, mapped and registered where the offsets agree mod 4 and the filesystem
    takes the registration, read through the ring otherwise (never asserted which: a filesystem may refuse)."""
    digests, paths, want = _layout(oracle, tmp_path)
    assert want == [int(i not in CORRUPT) for i in range(P)]
    bits, status, clock = _staged(native, digests, paths, FILE_DIRECT=1)
    print(clock)
    assert bits == want and status == [0] * 4
    assert clock["bytes_direct"] + clock["bytes_read"] == LONG, clock
    assert clock["bytes_read"] >= LONG - AGREE, clock       # the misaligned files' chunks are never mapped-direct
    assert clock["bytes_odirect"] == 0 and clock["odirect_fallbacks"] == 0, clock
    assert clock["small"] > 0, clock                         # (the 1,000-byte file: packed into a slot in the same call)


def test_warm_ring_reads(native, oracle, tmp_path):
    digests, paths, want = _layout(oracle, tmp_path)
    bits, status, clock = _staged(native, digests, paths, FILE_DIRECT=0)
    print(clock)
    assert bits == want and status == [0] * 4
    assert clock["bytes_direct"] == 0 and clock["bytes_odirect"] == 0, clock
    assert clock["bytes_read"] == LONG and clock["small"] > 0, clock
    assert clock["odirect_fallbacks"] == 0, clock


@pytest.mark.parametrize("bounce", [0, 2])
@pytest.mark.parametrize("odirect", [1, 2])
def test_cold_reads(native, oracle, tmp_path, odirect, bounce):
    """Files evicted from the page cache: file 0 (offsets agreeing mod 4) is read O_DIRECT into the ring (bounce = 0) or
    through the bounce buffers, the others buffered; with every O_DIRECT read refused (2) the same bits come through
    the counted fallback."""
    import fsutil
    digests, paths, want = _layout(oracle, tmp_path)

    def drop():
        assert fsutil.drop_cache(paths) <= 0.01

    bits, status, clock = _staged(native, digests, paths, before=drop, FILE_DIRECT=0, FILE_ODIRECT=odirect,
                                  FILE_BOUNCE=bounce)
    print(clock)
    assert bits == want and status == [0] * 4
    assert clock["bytes_direct"] == 0 and clock["bytes_read"] == LONG, clock
    if odirect == 1:
        assert clock["bytes_odirect"] == AGREE, clock
        assert clock["odirect_fallbacks"] == 0 and clock["odirect_errno"] == 0, clock
    else:
        assert clock["bytes_odirect"] == 0, clock
        assert clock["odirect_fallbacks"] > 0 and clock["odirect_errno"] == errno.EINVAL, clock


@pytest.mark.parametrize("cut", [0, 20000])
def test_streamed_equals_staged(native, oracle, tmp_path, cut):
    """tv_stream_file_table over the same files, warm and with TV_OPT_FILE_ODIRECT = 2: the staged call's bits and
    per-file statuses.  File 2 truncated by 20,000 bytes: the null pieces Storage.get gives, TV_ERR_IO for it alone."""
    digests, paths, want = _layout(oracle, tmp_path, cut)
    bits, status, _ = _staged(native, digests, paths, FILE_DIRECT=0)
    assert bits == want
    assert status == ([0, 0, native.TV_ERR_IO, 0] if cut else [0] * 4)
    if cut:
        first_null = (STARTS[2] + SIZES[2] - cut) // L
        assert want == [int(i not in CORRUPT and i < first_null) for i in range(P)]
    for odirect in (1, 2):
        sbits, sstatus, clock = _streamed(native, digests, paths, FILE_ODIRECT=odirect)
        print(odirect, clock)
        assert sbits == bits and sstatus == status, odirect
        assert clock["bytes_odirect"] == 0 and clock["odirect_fallbacks"] == 0, clock   # (warm: never O_DIRECT)
        if not cut:
            assert clock["bytes_read"] == TOTAL, clock


@pytest.mark.parametrize("odirect", [1, 2])
def test_streamed_cold_file_reads_o_direct(native, oracle, tmp_path, odirect):
    """The streamed reader's own O_DIRECT path, which the files above (under 1 MiB, warm) never reach: one cold file of
    1 MiB + 4,097 bytes through tv_stream_file_table.  With 1 every byte is read O_DIRECT (rows straight into the slot
    where aligned, through the reader's scratch where not, the last request short at the file's end); with 2 the reads
    are refused, counted, and the file reads buffered: the same bits."""
    import fsutil
    total = (1 << 20) + 4097
    pieces = -(-total // L)
    payload = bytes(oracle.synth_fill(92, 0, total))
    digests = bytearray(b"".join(hashlib.sha1(payload[i * L:min(total, (i + 1) * L)]).digest() for i in range(pieces)))
    digests[20 * 7] ^= 1
    digests[20 * (pieces - 1)] ^= 1
    path = tmp_path / "one.bin"
    path.write_bytes(payload)
    want = [int(i not in (7, pieces - 1)) for i in range(pieces)]
    with native.Context(0) as ctx:
        ctx.set_option(native.TV_OPT_RESIDENT, 0)
        ctx.set_option(native.TV_OPT_FILE_ODIRECT, odirect)
        ctx.set_layout(total, L, pieces)
        ctx.set_digests(bytes(digests))
        assert fsutil.drop_cache([str(path)]) <= 0.01
        ctx._reset_file_clock()
        bits, status = ctx.stream_file_table([total], [str(path)])
        clock = ctx._file_clock()
    print(clock)
    assert _bits(bits, pieces) == want and status == [0]
    assert clock["bytes_read"] == total, clock
    if odirect == 1:
        assert clock["bytes_odirect"] == total and clock["odirect_fallbacks"] == 0, clock
    else:
        assert clock["bytes_odirect"] == 0, clock
        # (readers that run side by side may each meet the refusal before the file is marked)
        assert clock["odirect_fallbacks"] > 0 and clock["odirect_errno"] == errno.EINVAL, clock
