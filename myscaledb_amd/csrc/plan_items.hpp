// The work items of a grouped plan (scan_kernels.hpp: IvfPlanParams) as records: plain C++, shared by the plan kernels that write the
// item table, the scan kernels that read it (or form the same record behind their binary search) and the host test.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSVS_HD __host__ __device__
#else
#define MSVS_HD
#endif

namespace msvs
{

/// Segments of a list of `blocks` 32-row blocks at a segment size of sb blocks (rounded to the nearest count, at least one;
/// an empty range has none), and the blocks per segment that go with it: shared by the plan kernel and the scan kernel.
MSVS_HD inline uint32_t plan_nseg(uint32_t blocks, uint32_t sb)
{
    if (blocks == 0)
        return 0;
    const uint32_t n = (blocks + sb / 2) / sb;
    return n ? n : 1;
}

/// One work item of a grouped plan over 32-row blocks: blocks [b_first, b_end) of list `list` (counted from the list's first
/// block, which is shadow block `hb`) against the pairs [pair_begin, pair_begin + nvalid) of one tile.  32 bytes, so that one
/// 32-byte (or two 16-byte) load fetches it; the row range in 32 bits (the shadow pass requires n <= 0xfffffff0).
struct alignas(32) IvfItem
{
    uint32_t list;
    uint32_t hb;            // first shadow block of the list (hoff[list])
    uint32_t b_first, b_end;
    uint32_t pair_begin, nvalid;
    uint32_t lbeg, lend;    // rows of the list the blocks are counted from: block b = rows [lbeg + 32 b, min(lbeg + 32 b + 32, lend))
};
static_assert(sizeof(IvfItem) == 32 && offsetof(IvfItem, hb) == 4 && offsetof(IvfItem, b_first) == 8 && offsetof(IvfItem, b_end) == 12
                  && offsetof(IvfItem, pair_begin) == 16 && offsetof(IvfItem, nvalid) == 20 && offsetof(IvfItem, lbeg) == 24,
              "the scan kernels read a record as two 16-byte words: {list, hb, b_first, b_end}, {pair_begin, nvalid, lbeg, lend}");

/// Work item w of list l.  Work order inside a list is [segment][tile] (tile fastest: the tiles of a segment are consecutive items).
/// work_l = work_off[l] <= w < work_off[l + 1]; [p0, pe) = the list's pairs, tiles of T; [b_lo, b_hi) = the 32-row blocks of the
/// partition's row range in the list; seg_blocks = 0: one segment, else segments of about seg_blocks blocks (plan_nseg).
MSVS_HD inline IvfItem ivf_make_item(uint32_t w, uint32_t l, uint32_t work_l, uint32_t p0, uint32_t pe, uint32_t b_lo, uint32_t b_hi,
                                     uint32_t seg_blocks, uint32_t T, uint32_t hb, uint32_t lbeg, uint32_t lend)
{
    const uint32_t t_in = w - work_l, ntiles = (pe - p0 + T - 1) / T;
    const uint32_t seg = t_in / ntiles, tidx = t_in - seg * ntiles;
    uint32_t b_first = b_lo, b_end = b_hi;
    if (seg_blocks)
    {
        const uint32_t blocks = b_hi - b_lo, nseg = plan_nseg(blocks, seg_blocks);
        const uint32_t per = (blocks + nseg - 1) / nseg;
        // (nseg is rounded to the nearest count, so the last segments of a list can come out empty: b_first = b_end = b_hi)
        b_first = seg * per < blocks ? b_lo + seg * per : b_hi;
        b_end = b_hi - b_first > per ? b_first + per : b_hi;
    }
    const uint32_t pb = p0 + tidx * T;
    return IvfItem{l, hb, b_first, b_end, pb, pe - pb < T ? pe - pb : T, lbeg, lend};
}

/// Work items of list l under a plan: tiles x segments (what the plan kernel's scan adds up in work_off).
MSVS_HD inline uint32_t ivf_list_items(uint32_t pairs, uint32_t blocks, uint32_t seg_blocks, uint32_t T)
{
    return ((pairs + T - 1) / T) * (seg_blocks ? plan_nseg(blocks, seg_blocks) : (blocks ? 1u : 0u));
}

/// Capacity of an item table that no plan over n_pairs pairs and nlist lists exceeds.  A list with c pairs has ceil(c / T) <=
/// floor(c / T) + 1 tiles, and only lists with pairs have any: sum of tiles <= floor(n_pairs / T) + min(nlist, n_pairs).  One
/// segment per list: that is the bound.  Segments chosen on the device (seg_target_items != 0): sb >= max(8, units / target) with
/// units = sum of tiles x blocks, and a list of b blocks has max(1, floor((b + sb / 2) / sb)) <= 1 + b / sb segments, so the items
/// are <= sum of tiles + units / sb <= sum of tiles + target.  (sb is capped at 2^30 blocks, above any list: one segment each.)
MSVS_HD inline uint64_t ivf_items_capacity(uint64_t n_pairs, uint64_t nlist, uint32_t T, uint32_t seg_target_items)
{
    return n_pairs / T + (nlist < n_pairs ? nlist : n_pairs) + seg_target_items;
}

} // namespace msvs
