"""Shared by the hybrid tests: hybrid .torrent fixtures with real BEP 47 pad entries, written with the tests' own
bencoder (tests/v2_util.py), and the expected values from hashlib (SHA-1 over the padded linear bytes) and tests/v2_ref.py
(the merkle side).  It shares no code with torrent_amd."""
from __future__ import annotations

import hashlib

from tests import v2_ref, v2_util


def pad_len(n: int, L: int) -> int:
    return -n % L


def padded_linear(files, L: int, trailing_pad: bool = False) -> bytes:
    """The v1 linear space of a hybrid torrent: every file followed by zeros up to the next piece boundary, except the
    last file that holds bytes (unless trailing_pad)."""
    last = max((k for k, d in enumerate(files) if len(d)), default=-1)
    out = bytearray()
    for k, d in enumerate(files):
        out += d
        if len(d) and (k != last or trailing_pad):
            out += bytes(pad_len(len(d), L))
    return bytes(out)


def v1_pieces(files, L: int, trailing_pad: bool = False) -> bytes:
    lin = padded_linear(files, L, trailing_pad)
    return b"".join(hashlib.sha1(lin[o:o + L]).digest() for o in range(0, len(lin), L))


def v2_expected(files, L: int) -> list:
    """The expected hash of every piece, in piece order."""
    out = []
    for d in files:
        out += v2_ref.file_hashes(d, L)[2]
    return out


def v1_file_list(files, paths, L: int, trailing_pad: bool = False) -> list:
    """The v1 `files` list with a pad entry after every file that does not end a piece and is followed by a file that
    holds bytes (and after the last one with trailing_pad)."""
    last = max((k for k, d in enumerate(files) if len(d)), default=-1)
    out = []
    for k, (comps, d) in enumerate(zip(paths, files)):
        out.append({"length": len(d), "path": list(comps)})
        n = pad_len(len(d), L)
        if n and len(d) and (k != last or trailing_pad):
            out.append({"attr": "p", "length": n, "path": [".pad", str(n)]})
    return out


def torrent_hybrid(files, L: int, name: str = "t", paths=None, trailing_pad: bool = False, pieces: bytes | None = None,
                   v1_files=None, single: bool = False, mutate=None) -> bytes:
    """A hybrid .torrent for `files` (bytes per file, file-tree order = list order).  pieces: the v1 `pieces` string
    (default: hashlib over the padded linear bytes).  v1_files: the v1 `files` list (default: v1_file_list).  single:
    one file described by `length` and `name`.  mutate(top) may edit the dictionary before it is encoded."""
    paths = [[name]] if single else (paths or v2_util.file_names(len(files)))

    def add_v1(top):
        info = top["info"]
        if single:
            info["length"] = len(files[0])
        else:
            info["files"] = v1_file_list(files, paths, L, trailing_pad) if v1_files is None else v1_files
        info["pieces"] = v1_pieces(files, L, trailing_pad) if pieces is None else pieces
        if mutate:
            mutate(top)

    return v2_util.torrent_v2(files, L, name=name, paths=paths, mutate=add_v1)


def bits(n: int, clear=()) -> bytes:
    return v2_util.set_bits(n, clear)
