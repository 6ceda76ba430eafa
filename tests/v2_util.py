"""Shared by the v2 tests: the golden layouts, their file bytes, and .torrent fixtures written with a small bencoder of
the tests' own (keys sorted, as canonical bencoding has them)."""
from __future__ import annotations

import functools
import json
import os

from tests import synth, v2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def benc(v) -> bytes:
    if isinstance(v, int):
        return b"i%de" % v
    if isinstance(v, str):
        v = v.encode()
    if isinstance(v, (bytes, bytearray)):
        return b"%d:" % len(v) + bytes(v)
    if isinstance(v, list):
        return b"l" + b"".join(benc(x) for x in v) + b"e"
    if isinstance(v, dict):
        items = sorted(((k.encode() if isinstance(k, str) else k), x) for k, x in v.items())
        return b"d" + b"".join(benc(k) + benc(x) for k, x in items) + b"e"
    raise TypeError(type(v))


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with open(os.path.join(ROOT, "tests", "golden", "v2_layouts.json")) as f:
        return {g["name"]: g for g in json.load(f)}


@functools.lru_cache(maxsize=None)
def golden_files(name: str) -> tuple:
    g = golden()[name]
    return tuple(bytes(synth.fill(g["seed"] + k, 0, n)) for k, n in enumerate(g["lengths"]))


def file_names(n: int) -> list:
    """Sorted names: the file-tree order is then the list order."""
    return [["d%02d" % (k // 3), "f%03d.bin" % k] for k in range(n)]


def torrent_v2(files, L: int, name: str = "t", paths=None, hybrid_pieces: bytes | None = None, mutate=None) -> bytes:
    """A v2 .torrent for `files` (bytes per file, file-tree order = list order) from the hashlib reference.  paths:
    path components per file (default file_names).  hybrid_pieces: also write the v1 keys with this `pieces` string.
    mutate(top) may edit the dictionary before it is encoded."""
    paths = paths or file_names(len(files))
    tree: dict = {}
    layers = {}
    for comps, data in zip(paths, files):
        root, layer, _ = v2_ref.file_hashes(data, L)
        node = tree
        for c in comps:
            node = node.setdefault(c, {})
        node[""] = {"length": len(data)} if root is None else {"length": len(data), "pieces root": root}
        if layer:
            layers[root] = layer
    info = {"file tree": tree, "meta version": 2, "name": name, "piece length": L}
    if hybrid_pieces is not None:
        # (pads zero: the hybrid fixtures use files that are whole multiples of L, or a single file)
        if len(files) == 1:
            info["length"] = len(files[0])
        else:
            info["files"] = [{"length": len(d), "path": list(c)} for c, d in zip(paths, files)]
        info["pieces"] = hybrid_pieces
    top = {"announce": "http://example.com/announce", "info": info, "piece layers": layers}
    if mutate:
        mutate(top)
    return benc(top)


def set_bits(n: int, clear=()) -> bytes:
    bf = bytearray((n + 7) // 8)
    for i in range(n):
        if i not in clear:
            bf[i >> 3] |= 0x80 >> (i & 7)
    return bytes(bf)
