"""sq_layout.hpp on the host alone: the stored order of an IVFSQ row at its three code widths.  A stand-alone program (own main)
against the header, built with the address and the undefined-behaviour sanitizer and run once.  For every dimension it checks that
each width's map is a bijection of the row's code slots, that the four codes of a float4 column stay together, and that the
columns of lane g (g, g + 16, ...) land in the lane's own 16-byte word of every whole block, and overall, in ascending order.
The program prints one line per (width, dim) and exits non-zero at the first wrong one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 5, 31, 64, 100, 127, 128, 129, 511, 512, 520, 768, 2240]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sq_layout.hpp"

using namespace msvs;

static bool fail_at(const char * what, uint32_t bits, uint32_t dim, uint32_t j)
{
    std::printf("FAIL bits %u dim %u: %s at %u\n", bits, dim, what, j);
    return false;
}

/// slot of natural column j in units of one code: bytes (8), nibbles (4), halves (16)
static uint32_t pos(uint32_t bits, uint32_t j, uint32_t ld)
{
    return bits == 8 ? sq_stored_pos(j, ld) : (bits == 4 ? sq4_stored_pos(j, ld) : sq16_stored_pos(j, ld));
}

static bool check(uint32_t bits, uint32_t dim)
{
    const uint32_t ld = (dim + 15) / 16 * 16, ld4 = ld / 4;
    const uint32_t row_bytes = 16 * sq_row_words(bits, ld);
    const uint32_t slots = row_bytes * 8 / bits;          // code slots of the stored row
    const uint32_t want_bytes = bits == 8 ? ld : (bits == 16 ? 2 * ld : ((dim + 1) / 2 + 15) / 16 * 16);
    if (row_bytes != want_bytes || slots < ld)
        return fail_at("row bytes", bits, dim, row_bytes);
    const uint32_t E = 32 / bits;                          // float4 columns of a lane per 16-byte word
    const uint32_t block_cols = 64 * E, nb = ld / block_cols; // natural columns of a whole block of 256 bytes; whole blocks
    // 1. a bijection: every column has a slot of its own inside the row ...
    std::vector<uint32_t> owner(slots, 0xffffffffu);
    for (uint32_t j = 0; j < ld; j++)
    {
        const uint32_t p = pos(bits, j, ld);
        if (p >= slots || owner[p] != 0xffffffffu)
            return fail_at("slot taken or outside the row", bits, dim, j);
        owner[p] = j;
    }
    // ... at 8 and 16 bits the columns fill the row; at 4 bits the inverse map names the columns of every stored byte, real and pad
    if (bits != 4)
    {
        if (slots != ld)
            return fail_at("slots", bits, dim, slots);
    }
    else
    {
        std::vector<uint8_t> seen(slots, 0);
        for (uint32_t p = 0; p < row_bytes; p++)
        {
            uint32_t lo, hi;
            sq4_stored_cols(p, ld, lo, hi);
            if (lo >= slots || hi >= slots || lo == hi || seen[lo] || seen[hi])
                return fail_at("inverse map: column repeated or beyond the row", bits, dim, p);
            seen[lo] = seen[hi] = 1;
            if ((lo < ld && sq4_stored_pos(lo, ld) != 2 * p) || (hi < ld && sq4_stored_pos(hi, ld) != 2 * p + 1))
                return fail_at("inverse map disagrees with the map", bits, dim, p);
            if ((lo >= ld && owner[2 * p] != 0xffffffffu) || (hi >= ld && owner[2 * p + 1] != 0xffffffffu))
                return fail_at("pad nibble owned by a column", bits, dim, p);
        }
    }
    // 2. the lane's columns: the four codes of a float4 column together, the lane's word in a block, ascending order
    for (uint32_t g = 0; g < 16; g++)
    {
        long last = -1;
        for (uint32_t c = g; c < ld4; c += 16)
        {
            const uint32_t p0 = pos(bits, 4 * c, ld);
            const bool in_block = 4 * c < nb * block_cols;
            const uint32_t stride = bits == 4 && in_block ? 2 : 1; // (a block keeps a column in one nibble plane of four bytes)
            for (uint32_t i = 1; i < 4; i++)
                if (pos(bits, 4 * c + i, ld) != p0 + stride * i)
                    return fail_at("a float4 column is split", bits, dim, c);
            // order key: the byte for 8 and 16 bits; at 4 bits (32-bit word, nibble plane, byte) inside a block
            long key = (long)p0 * bits / 8;
            if (bits == 4)
                key = in_block ? (long)(p0 / 2 / 4) * 8 + (p0 & 1) * 4 + (p0 / 2) % 4 : (long)p0;
            if (in_block)
            {
                const uint32_t b = 4 * c / block_cols, e = (c - b * (block_cols / 4)) / 16;
                const uint32_t byte = p0 * bits / 8;
                if (byte / 16 != 16 * b + g)
                    return fail_at("column outside its lane's 16-byte word", bits, dim, c);
                const uint32_t in_word = byte % 16;
                const uint32_t want = bits == 8 ? 4 * e : (bits == 16 ? 8 * e : 4 * (e / 2));
                if (in_word != want || (bits == 4 && (p0 & 1) != (e & 1)))
                    return fail_at("column out of its place in the lane's word", bits, dim, c);
            }
            else if (p0 != 4 * c)
                return fail_at("tail not in natural order", bits, dim, c);
            if (key <= last)
                return fail_at("lane's columns not ascending", bits, dim, c);
            last = key;
        }
    }
    std::printf("ok   bits %u dim %u: %u bytes, %u whole blocks\n", bits, dim, row_bytes, nb);
    return true;
}

int main()
{
    const uint32_t dims[] = {DIM_LIST};
    const uint32_t widths[] = {8, 4, 16};
    for (uint32_t bits : widths)
        for (uint32_t dim : dims)
            if (!check(bits, dim))
                return 1;
    return 0;
}
"""


def test_sq_layout_program(tmp_path):
    src = tmp_path / "sq_layout_test.cpp"
    exe = tmp_path / "sq_layout_test"
    src.write_text(PROGRAM.replace("DIM_LIST", ", ".join(str(d) for d in DIMS)))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "myscaledb_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * len(DIMS) and all(ln.startswith("ok") for ln in lines), r.stdout
