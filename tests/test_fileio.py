"""CPU unit tests of the file-read primitives in torrent_amd/csrc/tv_fileio.h (read_at, direct_request, read_direct,
pread_part) and of tv_plan.h's path-table parser, slot packing and copy runs, run through tests/c/fileio_main.cpp (an
ordinary executable: it also builds with -fsanitize=address,undefined).  Real files under tmp_path through buffered
descriptors: the rounding and the trimming do not depend on the open flag.  The expected values are restated here in
plain Python."""
import errno
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def fileio(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fileio") / "fileio_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "fileio_main.cpp"), "-o", exe])

    def run(queries):
        """queries: token lists -> one output line (split into tokens) per query."""
        text = "".join(" ".join(map(str, q)) + "\n" for q in queries)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        return [ln.split() for ln in lines]

    return run


def _read(tokens):
    """'count hex' -> (count, bytes); '-errno -' -> (-errno, b'')."""
    n = int(tokens[0])
    return n, (bytes.fromhex(tokens[1]) if n > 0 else b"")


@pytest.fixture(scope="module")
def blob_file(tmp_path_factory):
    def make(size, seed):
        p = tmp_path_factory.mktemp("data") / f"f{size}.bin"
        data = random.Random(seed).randbytes(size)
        p.write_bytes(data)
        return str(p), data
    return make


def test_read_loop(fileio, blob_file):
    path, data = blob_file(10_000, 1)
    cases = [(0, 100, 100), (123, 4096, 4096), (9_000, 1_000, 1_000),      # inside the file, and exactly to its end
             (9_000, 1_000, 4_096),                                         # ask > need at the end of the file
             (9_990, 10, 8_192), (9_000, 2_000, 2_000), (9_999, 4_096, 4_096),   # past the end: a short count, no error
             (10_000, 10, 10), (20_000, 10, 10),                            # wholly past it: 0
             (0, 0, 0), (5, 0, 4_096), (0, 10_000, 10_000), (0, 10_001, 12_288)]
    out = fileio([["r", path, off, need, ask] for off, need, ask in cases])
    for (off, need, ask), tok in zip(cases, out):
        n, got = _read(tok)
        if need == 0:
            assert n == 0, (off, need, ask)                                 # need = 0 reads nothing
            continue
        want = data[off:off + ask]      # the loop may take up to `ask` per request, and stops once `need` are in
        assert min(need, len(want)) <= n <= len(want), (off, need, ask)
        assert got == data[off:off + n], (off, need, ask)
        if off + need > len(data):
            assert n == len(data[off:off + need]), (off, need, ask)         # fewer than need: the file ended
    n, _ = _read(fileio([["x", path, 0, 10, 10]])[0])
    assert n == -errno.EBADF


def test_direct_request_rounding(fileio):
    cases = [(fo, n) for fo in range(0, 8201) for n in (1, 4095, 4096, 4097)]
    out = fileio([["q", fo, n] for fo, n in cases])
    for (fo, n), tok in zip(cases, out):
        al, lead, ask = map(int, tok)
        assert al <= fo and al % 4096 == 0 and ask % 4096 == 0 and lead == fo - al, (fo, n)
        assert lead < 4096
        assert ask >= lead + n > ask - 4096, (fo, n)                        # the least multiple covering lead + n


def test_read_direct_steps(fileio, blob_file):
    path, data = blob_file(40_001, 2)
    step = 8192
    cases = [(0, 4096), (0, 8192), (4096, 16384), (8192, 28672),            # aligned whole reads: the straight path
             (0, 40_960), (36_864, 8192),                                   # ... that end past the end of the file
             (1, 1), (5, 100), (4095, 2), (4097, 8191),                     # inside one step
             (100, 8192), (4000, 8193), (8191, 9000),                       # crossing into a second step
             (3, 16_385), (4095, 40_000 - 4095), (1, 40_000),               # three to five steps
             (7, 40_960), (39_000, 5_000), (40_000, 4096),                  # starts before, ends past the end
             (40_001, 10), (45_056, 4096), (50_001, 77), (0, 0)]            # wholly past the end; nothing
    out = fileio([["d", path, fo, n, step] for fo, n in cases])
    for (fo, n), tok in zip(cases, out):
        cnt, got = _read(tok)
        assert cnt == len(data[fo:fo + n]) and got == data[fo:fo + n], (fo, n)
    # the default step (4 MiB) reads the same bytes
    cnt, got = _read(fileio([["d", path, 3, 39_000, 4 << 20]])[0])
    assert got == data[3:39_003]


def test_pread_part(fileio):
    cases = [(n, t) for n in (1, 65_536, 1 << 20, (1 << 20) + 1, 33 << 20, (64 << 20) - 8192, 64 << 20, 1 << 30)
             for t in (0, 1, 2, 7, 8, 16)]
    out = fileio([["t", n, t] for n, t in cases])
    for (n, t), tok in zip(cases, out):
        part = n // (2 * max(1, t))
        part = -(-part // 65_536) * 65_536
        assert int(tok[0]) == min(4 << 20, max(1 << 20, part)), (n, t)


def _parse(fileio, n, blob):
    tok = fileio([["p", n, blob.hex() or "-"]])[0]
    k, offs = int(tok[0]), list(map(int, tok[1:]))
    assert len(offs) == k
    return k, [blob[o:blob.index(b"\0", o)] for o in offs]


def test_path_table_parser(fileio):
    assert _parse(fileio, 0, b"") == (0, [])
    assert _parse(fileio, 0, b"\0") == (0, [])
    for names in ([b"a"], [b"/x/one", b"two", b"dir/three.bin"], [b"a", b"", b"c"], [b"", b"", b""]):
        n = len(names)
        blob = b"\0".join(names) + b"\0"
        assert _parse(fileio, n, blob) == (n, blob.split(b"\0")[:n])
        # a buffer one NUL short / a paths_bytes that cuts the last NUL: the strings before it are found, not the last
        k, got = _parse(fileio, n, blob[:-1])
        assert k == n - 1 and got == names[:n - 1]
        # one path fewer than the table has files
        k, got = _parse(fileio, n + 1, blob)
        assert k == n and got == names
        # trailing bytes after the n-th string are ignored
        assert _parse(fileio, n, blob + b"tail\0more") == (n, names)
        assert _parse(fileio, n, blob + b"x") == (n, names)
    assert _parse(fileio, 2, b"") == (0, [])


def _pack(segs, slot):
    """The rule restated: slots of segments, each at the next offset that agrees with its linear offset mod 4; and per
    slot one copy per run of readable segments that follow each other in linear bytes."""
    out, i = [], 0
    while i < len(segs):
        used, j, packed = 0, i, []
        while j < len(segs):
            lin, ln, _ = segs[j]
            at = used + (lin - used) % 4
            if at + ln > slot:
                break
            packed.append(at)
            used = at + ln
            j += 1
        runs, q = [], i
        while q < j:
            if not segs[q][2]:
                q += 1
                continue
            r = q + 1
            while r < j and segs[r][2] and segs[r][0] == segs[r - 1][0] + segs[r - 1][1]:
                r += 1
            runs.append((q, r))
            q = r
        out.append((i, j, packed, runs))
        i = j
    return out


def _run_pack(fileio, segs, slot):
    tok = fileio([["s", slot, len(segs)] + [v for s in segs for v in s]])[0]
    out = []
    for group in " ".join(tok).split(";"):
        if not group.strip():
            continue
        left, _, right = group.partition("/")
        nums = list(map(int, left.split()))
        runs = [tuple(map(int, r.split(":"))) for r in right.split()]
        out.append((nums[0], nums[1], nums[2:], runs))
    return out


def test_slot_packing_and_copy_runs(fileio):
    slot = 300
    contiguous = lambda start, lens, ok=None: [(start + sum(lens[:k]), ln, 1 if ok is None else ok[k])  # noqa: E731
                                               for k, ln in enumerate(lens)]
    cases = []
    for res in range(4):                                   # linear offsets of every residue mod 4
        cases.append(contiguous(1000 + res, [10, 11, 12, 13, 14]))
        cases.append([(1000 + res, 50, 1), (2001 + 2 * res, 50, 1), (3002 + 3 * res, 7, 1)])
    cases.append(contiguous(400, [100, 200]))              # exactly fills the slot's remainder
    cases.append(contiguous(400, [100, 201]))              # a byte too long: the second slot
    cases.append(contiguous(401, [100, 199, 1]))           # ... with the alignment pad (401 % 4 = 1) counted
    cases.append(contiguous(401, [100, 198, 1, 1]))
    cases.append(contiguous(0, [40, 40, 40, 40], ok=[1, 0, 1, 1]))     # a failed segment inside a run: two copies
    cases.append(contiguous(0, [40, 40, 40], ok=[0, 1, 0]))
    cases.append(contiguous(0, [40, 40], ok=[0, 0]))
    cases.append([(0, 40, 1), (40, 40, 1), (81, 40, 1), (121, 10, 1)])  # a gap in linear offsets: a new run
    cases.append(contiguous(7, [300 - 3]))                 # one segment, a whole slot less its alignment
    cases.append(contiguous(3, [120] * 9))                 # several slots; runs never cross a slot
    rng = random.Random(5)
    for _ in range(40):
        segs, lin = [], rng.randrange(1 << 20)
        for _ in range(rng.randrange(1, 30)):
            ln = rng.randrange(1, slot - 3)
            segs.append((lin, ln, int(rng.random() < 0.8)))
            lin += ln + (rng.randrange(1, 9) if rng.random() < 0.3 else 0)
        cases.append(segs)
    for segs in cases:
        got = _run_pack(fileio, segs, slot)
        assert got == _pack(segs, slot), segs
        for i, j, packed, runs in got:                     # every byte at its linear offset's alignment, inside the slot
            for q, at in zip(range(i, j), packed):
                assert at % 4 == segs[q][0] % 4 and at + segs[q][1] <= slot
    assert len(_run_pack(fileio, contiguous(400, [100, 200]), slot)) == 1
    assert len(_run_pack(fileio, contiguous(400, [100, 201]), slot)) == 2
    assert _run_pack(fileio, contiguous(0, [40, 40, 40, 40], ok=[1, 0, 1, 1]), slot)[0][3] == [(0, 1), (2, 4)]
