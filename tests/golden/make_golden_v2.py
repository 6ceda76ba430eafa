"""Writes tests/golden/v2_layouts.json: seeded BitTorrent v2 layouts with their expected piece tables, piece hashes,
pieces roots, piece layers and bitfields, from hashlib (tests/v2_ref.py) and tests/synth.py alone.

    python tests/golden/make_golden_v2.py

File k of a layout holds synth.fill(seed + k, 0, length).  `missing` / `truncated` name one file that is absent /
cut to `keep` bytes (mid-piece) and the bitfield a verify must then give.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import synth, v2_ref  # noqa: E402

K = 1024
LAYOUTS = [
    # a zero-length file between two files, files of 1 byte, exactly L, L + 1, and 5 L + 16,385
    dict(name="multi64k", seed=101, L=64 * K, lengths=[3 * 64 * K + 100, 0, 1, 64 * K, 64 * K + 1, 5 * 64 * K + 16385,
                                                       40000], missing=4, truncated=(5, 2 * 64 * K + 20000)),
    # files 1, 2, 3 and 5 leaves long under L = 128 KiB (tree widths 1, 2, 4, 8), then a long file with a short last piece
    dict(name="small128k", seed=202, L=128 * K, lengths=[16384, 32768, 3 * 16384, 5 * 16384, 16385, 2 * 128 * K + 7 * 16384 + 1],
         missing=2, truncated=(5, 128 * K + 5)),
    # L = 16 KiB: every piece is one leaf
    dict(name="leaf16k", seed=303, L=16 * K, lengths=[16384 * 9 + 55, 56, 0, 0, 16383], missing=1, truncated=(0, 16384 * 4 + 1)),
]


def build(spec: dict) -> dict:
    L, lengths = spec["L"], spec["lengths"]
    files = [bytes(synth.fill(spec["seed"] + k, 0, n)) for k, n in enumerate(lengths)]
    roots, layers, hashes = [], {}, []
    for data in files:
        root, layer, piece_hashes = v2_ref.file_hashes(data, L)
        roots.append(root.hex() if root else None)
        if layer:
            layers[root.hex()] = layer.hex()
        hashes += piece_hashes
    table = v2_ref.piece_table(lengths, L)
    full = v2_ref.expected_bitfield(files, L, hashes)
    m = spec["missing"]
    t, keep = spec["truncated"]
    gone = list(files)
    gone[m] = None
    cut = list(files)
    cut[t] = files[t][:keep]
    return dict(name=spec["name"], seed=spec["seed"], piece_length=L, lengths=lengths, pieces_roots=roots,
                piece_layers=layers, piece_table=[list(r) for r in table], piece_hashes=[h.hex() for h in hashes],
                bitfield=full.hex(),
                missing=dict(file=m, bitfield=v2_ref.expected_bitfield(gone, L, hashes, have=lengths).hex()),
                truncated=dict(file=t, keep=keep, bitfield=v2_ref.expected_bitfield(cut, L, hashes, have=lengths).hex()))


if __name__ == "__main__":
    out = os.path.join(HERE, "v2_layouts.json")
    with open(out, "w") as f:
        json.dump([build(s) for s in LAYOUTS], f, indent=1)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")
