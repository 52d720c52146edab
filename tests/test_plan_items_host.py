"""plan_items.hpp on the host alone: a stand-alone program (own main) against the header that holds the item record and its
builder, built with the address and the undefined-behaviour sanitizer and run once.  For random small plans it enumerates every
work item and holds it against a plain restatement of the plan: every (segment, tile) of every list with pairs and rows exactly
once, the segments of a list a partition of its blocks, the tiles a partition of its pairs, and the table capacity never exceeded.
The program prints one line per configuration and exits non-zero at the first wrong one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "plan_items.hpp"

using namespace msvs;

static void check(bool ok, const char * what)
{
    if (!ok)
    {
        std::printf("FAIL %s\n", what);
        std::exit(1);
    }
}

struct List
{
    uint32_t pairs, rows;
};

/// One random plan: the main partition (blocks 1 .. of every list: block 0 is the sample launch's) when `main`, else the sample
/// partition (block 0 alone); segments chosen as the plan kernel chooses them when target != 0.  Returns the number of items.
static uint32_t one_plan(std::mt19937 & rng, uint32_t T, uint32_t target, bool main_part)
{
    static const uint32_t lens[] = {0, 1, 32, 33, 64, 65, 200, 1000, 4000, 20000}, cnts[] = {0, 0, 1, 31, 32, 33, 95, 96, 97, 300};
    const uint32_t nlist = 1 + rng() % 40;
    std::vector<List> L(nlist);
    uint64_t n_pairs = 0, units = 0;
    for (List & l : L)
    {
        l = {cnts[rng() % 10], lens[rng() % 10]};
        if (rng() % 4 == 0)
            l.rows += rng() % 40;
        n_pairs += l.pairs;
    }
    auto b_lo = [&](const List & l) { return main_part && l.rows > 0 ? 1u : 0u; };
    auto blocks = [&](const List & l) {
        const uint32_t all = (l.rows + 31) / 32;
        return main_part ? (all ? all - 1 : 0u) : (all ? 1u : 0u);
    };
    for (const List & l : L)
        units += (uint64_t)((l.pairs + T - 1) / T) * blocks(l);
    uint32_t sb = 0;
    if (target)
    {
        const uint64_t per = (units + target - 1) / target;
        sb = std::max<uint32_t>(8, (uint32_t)((per + 7) / 8 * 8));
    }
    std::vector<uint32_t> work_off(nlist + 1, 0), pair_off(nlist + 1, 0), hoff(nlist + 1, 0), row_off(nlist + 1, 0);
    for (uint32_t l = 0; l < nlist; l++)
    {
        work_off[l + 1] = work_off[l] + ivf_list_items(L[l].pairs, blocks(L[l]), sb, T);
        pair_off[l + 1] = pair_off[l] + L[l].pairs;
        hoff[l + 1] = hoff[l] + (L[l].rows + 31) / 32;
        row_off[l + 1] = row_off[l] + L[l].rows;
    }
    const uint32_t total = work_off[nlist];
    check(total <= ivf_items_capacity(n_pairs, nlist, T, target), "the capacity bound");
    uint32_t w = 0;
    for (uint32_t l = 0; l < nlist; l++)
    {
        const uint32_t c = L[l].pairs, nb = blocks(L[l]), lo = b_lo(L[l]);
        if (c == 0 || nb == 0)
        {
            check(work_off[l + 1] == work_off[l], "a list without pairs or rows has no item");
            continue;
        }
        // the plain restatement: segments of `per` blocks from lo on, tiles of T pairs
        const uint32_t ntiles = (c + T - 1) / T;
        uint32_t nseg = 1;
        if (sb)
            nseg = std::max<uint32_t>(1, (nb + sb / 2) / sb);
        const uint32_t per = (nb + nseg - 1) / nseg;
        check(work_off[l + 1] - work_off[l] == nseg * ntiles, "items of a list = segments x tiles");
        std::vector<uint32_t> block_seen(nb, 0);
        for (uint32_t seg = 0; seg < nseg; seg++)
        {
            const uint32_t s_lo = std::min<uint64_t>((uint64_t)seg * per, nb), s_hi = std::min<uint64_t>((uint64_t)seg * per + per, nb);
            std::vector<uint32_t> pair_seen(c, 0);
            for (uint32_t t = 0; t < ntiles; t++, w++)
            {
                check(w < work_off[l + 1], "work order: [segment][tile] inside the list");
                const IvfItem it = ivf_make_item(w, l, work_off[l], pair_off[l], pair_off[l + 1], lo, lo + nb, sb, T, hoff[l], row_off[l], row_off[l + 1]);
                check(it.list == l && it.hb == hoff[l] && it.lbeg == row_off[l] && it.lend == row_off[l + 1], "the list's own fields");
                check(it.b_first == lo + s_lo && it.b_end == lo + s_hi && it.b_first <= it.b_end, "the segment's blocks");
                check(it.pair_begin == pair_off[l] + t * T && it.nvalid == std::min(T, c - t * T) && it.nvalid >= 1, "the tile's pairs");
                for (uint32_t i = 0; i < it.nvalid; i++)
                    pair_seen[it.pair_begin - pair_off[l] + i]++;
                if (t == 0)
                    for (uint32_t b = it.b_first; b < it.b_end; b++)
                        block_seen[b - lo]++;
            }
            check(std::all_of(pair_seen.begin(), pair_seen.end(), [](uint32_t v) { return v == 1; }), "the tiles partition the pairs");
        }
        check(std::all_of(block_seen.begin(), block_seen.end(), [](uint32_t v) { return v == 1; }), "the segments partition the blocks");
    }
    check(w == total, "every item enumerated once");
    return total;
}

int main()
{
    static_assert(sizeof(IvfItem) == 32 && alignof(IvfItem) == 32, "one aligned 32-byte record");
    check(plan_nseg(0, 8) == 0 && plan_nseg(3, 8) == 1 && plan_nseg(11, 8) == 1 && plan_nseg(12, 8) == 2 && plan_nseg(801, 8) == 100, "plan_nseg");
    {
        // 801 blocks in segments of 8: 100 segments of 9 blocks, the last eleven empty
        const IvfItem a = ivf_make_item(88, 0, 0, 0, 5, 1, 802, 8, 32, 7, 100, 100 + 802 * 32);
        const IvfItem b = ivf_make_item(89, 0, 0, 0, 5, 1, 802, 8, 32, 7, 100, 100 + 802 * 32);
        check(a.b_first == 793 && a.b_end == 802 && b.b_first == 802 && b.b_end == 802 && b.nvalid == 5, "empty last segments");
    }
    std::mt19937 rng(11);
    const uint32_t Ts[] = {32, 96}, targets[] = {0, 4, 64, 1024};
    for (const uint32_t T : Ts)
        for (const uint32_t target : targets)
            for (int main_part = 1; main_part >= (target ? 1 : 0); main_part--)
            {
                uint64_t items = 0;
                for (int rep = 0; rep < 300; rep++)
                    items += one_plan(rng, T, target, main_part != 0);
                std::printf("ok   T = %u, segment target %u, %s partition: 300 plans, %llu items\n", T, target, main_part ? "main" : "sample",
                            (unsigned long long)items);
            }
    return 0;
}
"""


def test_plan_items_program(tmp_path):
    src = tmp_path / "plan_items_test.cpp"
    exe = tmp_path / "plan_items_test"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "myscaledb_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 10 and all(ln.startswith("ok") for ln in lines), r.stdout
