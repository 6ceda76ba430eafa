// tv_fileio.h -- the file-read primitives of tv_files.hip and tv_stream.hip's row reader.  POSIX only (no HIP, no
// tv_ctx): unit-tested on the CPU (tests/test_fileio.py).  What a short read means stays with the callers.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>

namespace tvi {

// Read from `fd` at `off` into `dst`, asking for up to `ask` bytes, until at least `need` bytes are in; EINTR is
// retried.  -> the bytes read (fewer than `need`: the file ended), or -errno (*done: the bytes read before it).  (ask >
// need: an O_DIRECT request rounded up past the file's end comes back short, complete, and must not be continued.)
inline int64_t read_at(int fd, uint8_t* dst, uint64_t off, uint64_t need, uint64_t ask, uint64_t* done = nullptr) {
    uint64_t o = 0;
    int err = 0;
    while (o < need) {
        const ssize_t got = pread(fd, dst + o, ask - o, (off_t)(off + o));
        if (got < 0 && errno == EINTR) continue;
        if (got < 0) err = errno;
        if (got <= 0) break;
        o += (uint64_t)got;
    }
    if (done) *done = o;
    return err ? -(int64_t)err : (int64_t)o;
}

// The O_DIRECT request that covers file bytes [fo, fo + n): `ask` bytes of whole 4 KiB blocks from `al` (<= fo); the
// bytes wanted start `lead` bytes into what comes back.
struct DirectReq {
    uint64_t al, lead, ask;
};
inline DirectReq direct_request(uint64_t fo, uint64_t n) {
    const uint64_t al = fo / 4096 * 4096, lead = fo - al;
    return {al, lead, (lead + n + 4095) / 4096 * 4096};
}

// The file at `path` opened O_DIRECT with the access mode its first open had (< 0: the filesystem does not take it).
inline int open_direct(const char* path, bool rw) { return open(path, (rw ? O_RDWR : O_RDONLY) | O_DIRECT | O_CLOEXEC); }

// File bytes [fo, fo + len) -> dst through the O_DIRECT descriptor: straight into dst when the file offset, dst and
// the length are 4 KiB-aligned (whole-row reads of a one-file torrent), else via a 4 KiB-aligned scratch of the
// calling thread's in steps of `step` bytes.  -> bytes read (short: the file ended), or -errno.
inline int64_t read_direct(int dfd, uint64_t fo, uint8_t* dst, uint64_t len, uint64_t step = 4ull << 20) {
    if (fo % 4096 == 0 && (uintptr_t)dst % 4096 == 0 && len % 4096 == 0) return read_at(dfd, dst, fo, len, len);
    struct Scratch {   // (sized to the longest read the thread has needed: a row, at most step + 8 KiB)
        uint8_t* p = nullptr;
        uint64_t cap = 0;
        ~Scratch() { free(p); }
    };
    thread_local Scratch scratch;
    const uint64_t cap = std::min(step, len) + 8192;
    if (scratch.cap < cap) {
        free(scratch.p);
        scratch.cap = 0;
        if (posix_memalign((void**)&scratch.p, 4096, cap)) {
            scratch.p = nullptr;
            return -ENOMEM;
        }
        scratch.cap = cap;
    }
    for (uint64_t o = 0; o < len;) {
        const uint64_t m = std::min(step, len - o);
        const DirectReq r = direct_request(fo + o, m);
        const int64_t got = read_at(dfd, scratch.p, r.al, r.ask, r.ask);
        if (got < 0) return got;
        const uint64_t have = (uint64_t)got > r.lead ? std::min(m, (uint64_t)got - r.lead) : 0;
        memcpy(dst + o, scratch.p + r.lead, have);
        o += have;
        if (have < m) return (int64_t)o;   // the file ended
    }
    return (int64_t)len;
}

// The part size of a pooled read of n bytes on `threads` threads: 1-4 MiB, a multiple of 64 KiB, at least two parts
// per thread so the slowest part ends the read early.
inline uint64_t pread_part(uint64_t n, int threads) {
    const uint64_t part = n / (2 * (uint64_t)std::max(1, threads));
    return std::min<uint64_t>(4ull << 20, std::max<uint64_t>(1ull << 20, (part + 65535) / 65536 * 65536));
}

}  // namespace tvi
