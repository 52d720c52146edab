"""list_layout.hpp on the host alone: a stand-alone program (own main) against the header, built with the address and the
undefined-behaviour sanitizer and run once.  The program prints one line per case and exits non-zero at the first wrong one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
#include "list_layout.hpp"

using namespace msvs;

static void check(bool ok, const char * what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok)
        std::exit(1);
}

struct Row
{
    int32_t list;
    uint32_t id, pos;
};

/// the reference: a stable sort by (list, id) of the rows in staged order, counts, prefix sum
static bool same_as_stable_sort(const std::vector<int32_t> & list, const std::vector<uint32_t> & id, size_t nlist)
{
    const size_t n = list.size();
    std::vector<Row> rows(n);
    for (size_t i = 0; i < n; i++)
        rows[i] = {list[i], id[i], (uint32_t)i};
    std::stable_sort(rows.begin(), rows.end(), [](const Row & a, const Row & b) { return a.list != b.list ? a.list < b.list : a.id < b.id; });
    std::vector<int64_t> off(nlist + 1, 0);
    size_t longest = 0;
    for (const Row & r : rows)
        off[r.list + 1]++;
    for (size_t l = 0; l < nlist; l++)
    {
        longest = std::max<size_t>(longest, (size_t)off[l + 1]);
        off[l + 1] += off[l];
    }
    const ListLayout got = list_major_layout(list.data(), id.data(), n, nlist);
    if (got.order.size() != n || got.list_off != off || got.max_list_len != longest)
        return false;
    for (size_t p = 0; p < n; p++)
        if (got.order[p] != rows[p].pos)
            return false;
    return longest_list(got.list_off) == longest && list_offsets_error(got.list_off, n, "x").empty();
}

int main()
{
    {
        const ListLayout e = list_major_layout((const int32_t *)nullptr, (const uint32_t *)nullptr, 0, 3);
        check(e.order.empty() && e.list_off == std::vector<int64_t>{0, 0, 0, 0} && e.max_list_len == 0, "0 rows");
    }
    {
        const std::vector<int32_t> list{0, 0, 0, 0};
        const std::vector<uint32_t> id{7, 3, 9, 1};
        const ListLayout one = list_major_layout(list.data(), id.data(), 4, 1);
        check(one.order == std::vector<uint32_t>{3, 1, 0, 2} && one.list_off == std::vector<int64_t>{0, 4} && one.max_list_len == 4, "one list");
        check(same_as_stable_sort(list, id, 1), "one list against the stable sort");
    }
    {
        const std::vector<int32_t> list{3, 0, 2, 0, 3, 3};
        const std::vector<uint32_t> id{5, 9, 1, 2, 4, 0xfffffffeu};
        const ListLayout g = list_major_layout(list.data(), id.data(), 6, 5);
        check(g.order == std::vector<uint32_t>{3, 1, 2, 4, 0, 5} && g.list_off == std::vector<int64_t>{0, 2, 2, 3, 6, 6} && g.max_list_len == 3,
              "nlist = 5, lists 1 and 4 empty");
        check(same_as_stable_sort(list, id, 5), "nlist = 5 against the stable sort");
    }
    {
        const std::vector<int32_t> list{1, 0, 1, 1, 0, 1};
        const std::vector<uint32_t> id{4, 8, 4, 2, 8, 4};
        const ListLayout d = list_major_layout(list.data(), id.data(), 6, 2);
        check(d.order == std::vector<uint32_t>{1, 4, 3, 0, 2, 5}, "duplicate ids: the staged order breaks the tie");
        check(same_as_stable_sort(list, id, 2), "duplicate ids against the stable sort");
    }
    {
        std::mt19937 rng(5);
        std::vector<int32_t> list(1000);
        std::vector<uint32_t> id(1000);
        for (size_t i = 0; i < 1000; i++)
        {
            list[i] = (int32_t)(rng() % 37);
            id[i] = rng() % 50 == 0 ? 0xfffffff0u - rng() % 3 : rng() % 200; // few distinct ids: many ties
        }
        check(same_as_stable_sort(list, id, 37), "1000 random rows against the stable sort");
        check(same_as_stable_sort(list, id, 40), "the last lists empty");
        const std::vector<uint32_t> ulist(list.begin(), list.end()); // the binary index keeps its lists unsigned
        check(list_major_layout(ulist.data(), id.data(), 1000, 37).order == list_major_layout(list.data(), id.data(), 1000, 37).order,
              "unsigned list numbers");
    }
    const char * what = "msvs IVFSQ index";
    check(list_offsets_error({1, 2, 5}, 5, what) == "corrupt msvs IVFSQ index: the list offsets do not span the rows", "first offset != 0");
    check(list_offsets_error({0, 2, 4}, 5, what) == "corrupt msvs IVFSQ index: the list offsets do not span the rows", "last offset != n");
    check(list_offsets_error({0, 4, 3, 5}, 5, what) == "corrupt msvs IVFSQ index: descending list offsets", "one descending step");
    check(list_offsets_error({0, 0, 0, 0}, 0, what).empty() && longest_list({0, 0, 0, 0}) == 0, "all lists empty, n = 0");
    check(list_offsets_error({0, 2, 2, 5}, 5, what).empty() && longest_list({0, 2, 2, 5}) == 3, "valid offsets");
    return 0;
}
"""


def test_list_layout_program(tmp_path):
    src = tmp_path / "list_layout_test.cpp"
    exe = tmp_path / "list_layout_test"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "myscaledb_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 15 and all(ln.startswith("ok") for ln in lines), r.stdout
