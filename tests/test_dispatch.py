"""dispatch.hpp on the host alone: a stand-alone program (own main) against the header, built with the address and the
undefined-behaviour sanitizer and run once.  The program prints one line per case and exits non-zero at the first wrong one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dispatch.hpp"

using namespace msvs;

constexpr int M_L2 = 0, M_IP = 1; // scan_kernels.hpp (which needs HIP)

static void check(bool ok, const char * what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok)
        std::exit(1);
}

/// every listed value reaches its own constant, 0 / -1 / 3 / INT_MAX (where unlisted) and every other unlisted value of
/// -2 .. 40 reach the last one, and f runs exactly once per call
template <int... V>
static bool list_ok()
{
    const std::vector<int> listed{V...};
    std::vector<int> probe{0, -1, 3, INT_MAX, INT_MIN};
    for (int v = -2; v <= 40; v++)
        probe.push_back(v);
    for (int v : probe)
    {
        int want = listed.back();
        for (int l : listed)
            if (l == v)
                want = l;
        int calls = 0, got = INT_MIN;
        with_int<V...>(v, [&](auto c) {
            calls++;
            got = decltype(c)::value;
        });
        if (calls != 1 || got != want)
            return false;
    }
    return true;
}

template <int A, int B, int C>
struct Triple
{
    static int code() { return A * 10000 + B * 100 + C; }
};

int main()
{
    check(list_ok<1, 2, 4>(), "<1, 2, 4>");
    check(list_ok<2, 4, 8>(), "<2, 4, 8>: no T = 1, 1 takes 8");
    check(list_ok<1, 2, 4, 8>(), "<1, 2, 4, 8>");
    check(list_ok<1, 2, 4, 8, 16>(), "<1, 2, 4, 8, 16>");
    check(list_ok<1, 2, 3, 4>(), "<1, 2, 3, 4>");
    check(list_ok<M_IP, M_L2>(), "<M_IP, M_L2>: cosine (2) takes M_L2's branch as the else did");
    check(list_ok<7>(), "a single value takes everything");
    {
        int got = -1;
        with_int<2, 4, 8>(1, [&](auto c) { got = decltype(c)::value; });
        check(got == 8, "T = 1 on <2, 4, 8> reaches 8, not 2");
        with_int<1, 2, 3, 4>(5, [&](auto c) { got = decltype(c)::value; });
        check(got == 4, "ncb = 5 on <1, 2, 3, 4> reaches 4");
        with_int<1, 2, 4, 8, 16>(3, [&](auto c) { got = decltype(c)::value; });
        check(got == 16, "g = 3 on <1, 2, 4, 8, 16> reaches 16");
    }
    {
        int calls = 0, t = 0, f = 0;
        with_bool(true, [&](auto b) {
            calls++;
            t = decltype(b)::value ? 1 : 2;
        });
        with_bool(false, [&](auto b) {
            calls++;
            f = decltype(b)::value ? 1 : 2;
        });
        check(calls == 2 && t == 1 && f == 2, "with_bool");
    }
    {
        // three nested levels, the constants as template arguments of the innermost call: the launchers' form
        bool ok = true;
        int calls = 0;
        for (int m : {M_IP, M_L2, 2})
            for (int t : {1, 2, 4, 8, 3})
                for (int k : {1, 64, 65, 128, 129, 256})
                {
                    int code = -1;
                    with_int<M_IP, M_L2>(m, [&](auto mc) {
                        with_int<2, 4, 8>(t, [&](auto tc) {
                            with_int<1, 2, 4>(r_for_k((uint32_t)k), [&](auto rc) {
                                calls++;
                                code = Triple<decltype(mc)::value, decltype(tc)::value, decltype(rc)::value>::code();
                            });
                        });
                    });
                    const int wm = m == M_IP ? M_IP : M_L2, wt = t == 2 || t == 4 ? t : 8, wr = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
                    ok = ok && code == wm * 10000 + wt * 100 + wr;
                }
        check(ok && calls == 3 * 5 * 6, "three nested levels, once each");
    }
    check(r_for_k(1) == 1 && r_for_k(64) == 1, "r_for_k: 1, 64 -> 1");
    check(r_for_k(65) == 2 && r_for_k(128) == 2, "r_for_k: 65, 128 -> 2");
    check(r_for_k(129) == 4 && r_for_k(256) == 4, "r_for_k: 129, 256 -> 4");
    return 0;
}
"""


def test_dispatch_program(tmp_path):
    src = tmp_path / "dispatch_test.cpp"
    exe = tmp_path / "dispatch_test"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "myscaledb_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 15 and all(ln.startswith("ok") for ln in lines), r.stdout
