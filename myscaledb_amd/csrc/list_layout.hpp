// list_layout.hpp -- the list-major layout of a partitioned index on the host: the order of its rows, the list offsets, and the
// check of offsets that come from a file.  Plain C++17 (no HIP): one definition for the float IVFFLAT, the IVFSQ and the
// partitioned binary index.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace msvs
{

struct ListLayout
{
    std::vector<uint32_t> order;   // order[p]: staged position of the row that sits at list-major position p
    std::vector<int64_t> list_off; // [nlist + 1]
    size_t max_list_len = 0;
};

/// n rows in staged order with their list (in [0, nlist)) and id -> the stable list-major order: by list, then id, then staged
/// position.  The position is part of the sort key, so the keys are unique and a plain sort gives what a stable sort by
/// (list, id) gives.  n < 2^32.
template <typename L>
inline ListLayout list_major_layout(const L * list, const uint32_t * id, size_t n, size_t nlist)
{
    ListLayout out;
    out.list_off.assign(nlist + 1, 0);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (size_t i = 0; i < n; i++)
    {
        keyed[i] = {(uint64_t)(uint32_t)list[i] << 32 | id[i], (uint32_t)i};
        out.list_off[(size_t)list[i] + 1]++;
    }
    std::sort(keyed.begin(), keyed.end());
    out.order.resize(n);
    for (size_t p = 0; p < n; p++)
        out.order[p] = keyed[p].second;
    for (size_t l = 0; l < nlist; l++)
    {
        out.max_list_len = std::max<size_t>(out.max_list_len, (size_t)out.list_off[l + 1]);
        out.list_off[l + 1] += out.list_off[l];
    }
    return out;
}

/// rows of the longest list of ascending offsets
inline size_t longest_list(const std::vector<int64_t> & off)
{
    size_t longest = 0;
    for (size_t l = 0; l + 1 < off.size(); l++)
        longest = std::max<size_t>(longest, (size_t)(off[l + 1] - off[l]));
    return longest;
}

/// List offsets read from a file must start at 0, end at n and never descend: "" if they do, else the error text about the
/// index kind `what` ("msvs IVFSQ index").
inline std::string list_offsets_error(const std::vector<int64_t> & off, size_t n, const char * what)
{
    if (off.empty() || off.front() != 0 || off.back() != (int64_t)n)
        return std::string("corrupt ") + what + ": the list offsets do not span the rows";
    for (size_t l = 0; l + 1 < off.size(); l++)
        if (off[l + 1] < off[l])
            return std::string("corrupt ") + what + ": descending list offsets";
    return std::string();
}

}
