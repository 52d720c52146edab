// io_stream.hpp -- a named file of an index file set, opened through the caller's msvs_io_t (include/msvs.h: the host's
// IndexDataFileWriter / IndexDataFileReader stream openers, VectorIndexIO.h:25-166); shared by the float and the binary index.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/msvs.h"
#include "common.hpp"

namespace msvs
{

constexpr size_t IO_CHUNK = (size_t)64 << 20;

struct IoStream
{
    const msvs_io_t * io;
    void * h;
    const char * name;
    IoStream(const msvs_io_t * io_, const char * name_, int write) : io(io_), h(nullptr), name(name_)
    {
        if (!io || !io->open || !io->close || (write ? !io->write : !io->read))
            fail(MSVS_ERR_INVALID_ARGUMENT, "msvs_io_t lacks a callback");
        h = io->open(io->ctx, name, write);
        if (!h)
            fail(MSVS_ERR_IO, "cannot open index file `%s` for %s", name, write ? "writing" : "reading");
    }
    ~IoStream()
    {
        if (h)
            (void)io->close(io->ctx, h);
    }
    void write(const void * p, size_t n)
    {
        const char * c = static_cast<const char *>(p);
        while (n)
        {
            const size_t m = std::min(n, IO_CHUNK);
            if (io->write(io->ctx, h, c, m) != (int64_t)m)
                fail(MSVS_ERR_IO, "short write to index file `%s`", name);
            c += m;
            n -= m;
        }
    }
    void read(void * p, size_t n)
    {
        char * c = static_cast<char *>(p);
        while (n)
        {
            const int64_t got = io->read(io->ctx, h, c, std::min(n, IO_CHUNK));
            if (got <= 0)
                fail(MSVS_ERR_IO, "index file `%s` is truncated", name);
            c += got;
            n -= (size_t)got;
        }
    }
    void finish()
    {
        void * t = h;
        h = nullptr;
        if (io->close(io->ctx, t) != 0)
            fail(MSVS_ERR_IO, "closing index file `%s` failed", name);
    }
};

/// `count` values of a file section in pieces of 64 MB: the buffer grows with what has really been read, so a corrupt or truncated
/// file ends in MSVS_ERR_IO (a short read) instead of an allocation sized by an untrusted header
template <typename V>
inline void read_grow(IoStream & f, std::vector<V> & v, size_t count)
{
    const size_t piece = IO_CHUNK / sizeof(V);
    for (size_t got = 0; got < count;)
    {
        const size_t m = std::min(piece, count - got);
        v.resize(got + m);
        f.read(v.data() + got, m * sizeof(V));
        got += m;
    }
}

inline void expect_end(IoStream & f)
{
    char c;
    if (f.io->read(f.io->ctx, f.h, &c, 1) > 0)
        fail(MSVS_ERR_IO, "index file `%s` is longer than its header says", f.name);
}

/// FNV-1a over n bytes: the check word of a file header
inline uint64_t fnv1a(const void * p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++)
        h = (h ^ static_cast<const unsigned char *>(p)[i]) * 0x100000001b3ull;
    return h;
}

}
