"""CPU unit tests of the digest-word codec in torrent_amd/csrc/tv_plan.h (digest_pack, digest_unpack), run through
tests/c/plan_codec_main.cpp (an ordinary executable: it also builds with -fsanitize=address,undefined).  The library
keeps every digest as big-endian 32-bit values, struct of arrays: word k of the digest in column `col` of a table of
row length `pitch` is table[k * pitch + col].  The expected values are restated here in plain Python; the forms are
the ones the calls use: pitch = count (tv_set_digests), a pitch larger than the count and a base inside a larger table
(tv_v2_set_pieces), and a stream's window-packed table (pitch = the window's count, base 8 * j0)."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xEEEEEEEE

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_codec") / "plan_codec_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "plan_codec_main.cpp"), "-o", exe])

    def run(words, tabwords, places, digests):
        """places: (base, pitch, col) per digest -> (the table's words, the digests unpacked again)."""
        tok = ["c", words, tabwords, len(places)] + [v for p in places for v in p] + [b"".join(digests).hex() or "-"]
        r = subprocess.run([exe], input=" ".join(map(str, tok)) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        tab, _, out = r.stdout.strip().partition("|")
        out = bytes.fromhex(out.strip())
        n = 4 * words
        return [int(w, 16) for w in tab.split()], [out[i:i + n] for i in range(0, len(out), n)]

    return run


def expected_table(words, tabwords, places, digests):
    tab = [SENTINEL] * tabwords
    for (base, pitch, col), d in zip(places, digests):
        for k in range(words):
            tab[base + k * pitch + col] = int.from_bytes(d[4 * k:4 * k + 4], "big")
    return tab


def draw(rng, words, count):
    out = [rng.randbytes(4 * words) for _ in range(count)]
    if count:
        out[0] = bytes(range(1, 4 * words + 1))      # every byte distinct: a swapped byte or word shows
    return out


@pytest.mark.parametrize("words", [5, 8])
@pytest.mark.parametrize("count", [0, 1, 3, 64, 65])
def test_pack_and_unpack(codec, words, count):
    rng = random.Random(words * 100 + count)
    digests = draw(rng, words, count)
    for pitch, base in ((count, 0), (count + 7, 0), (count + 3, 2 * (count + 3))):   # the last: rows 2.. of a larger table
        if count == 0 and pitch == 0:
            assert codec(words, 1, [], []) == ([SENTINEL], [])
            continue
        places = [(base, pitch, j) for j in range(count)]
        tabwords = base + words * pitch + 1
        tab, back = codec(words, tabwords, places, digests)
        assert tab == expected_table(words, tabwords, places, digests), (pitch, base)
        assert back == digests
        # the words of other columns, of the rows before the base and past the table's end: untouched
        written = {base + k * pitch + j for k in range(words) for j in range(count)}
        assert all(tab[i] == SENTINEL for i in range(tabwords) if i not in written)


@pytest.mark.parametrize("count,wn", [(5, 3), (65, 64), (130, 64), (7, 7), (3, 1)])
def test_window_packed_table(codec, count, wn):
    """A v2 stream's expected rows: window after window, each a table of its own at 8 * j0 whose row length is the
    window's piece count (the last window's may be smaller)."""
    words = 8
    digests = draw(random.Random(count), words, count)
    places = []
    for j in range(count):
        j0 = j // wn * wn
        places.append((8 * j0, min(wn, count - j0), j - j0))
    tab, back = codec(words, 8 * count + 1, places, digests)
    assert tab == expected_table(words, 8 * count + 1, places, digests)
    # the windows tile the table: every word is written exactly once, and nothing after it
    assert sorted(b + k * p + c for b, p, c in places for k in range(words)) == list(range(8 * count))
    assert tab[-1] == SENTINEL and back == digests
    # restated from the reader's side: window w's launches read word k of its piece q at 8 * j0 + k * wcount + q
    for j0 in range(0, count, wn):
        wcount = min(wn, count - j0)
        for q in range(wcount):
            got = b"".join(tab[8 * j0 + k * wcount + q].to_bytes(4, "big") for k in range(words))
            assert got == digests[j0 + q]


def test_scattered_destination(codec):
    """tv_v2_leaf_hashes: item t of m unpacks to (entry * W + leaf) * 32 of the output; here the order is reversed, so
    the program's contiguous output holds the digests of columns m-1 .. 0."""
    words, m = 8, 6
    digests = draw(random.Random(9), words, m)
    places = [(0, m, m - 1 - t) for t in range(m)]
    tab, back = codec(words, words * m, places, digests)
    assert back == digests
    assert tab == expected_table(words, words * m, places, digests)
