// The (u32 cell key, 16-byte record) sorts of the fp32 ICP index build (grid.hip) and of the ICP
// query set (icp_create.hip) keep rocPRIM's tuned gfx950 default (8 key bits per pass: 4 passes for
// the ~30-bit cell keys).  Also the one helper every plain sort site uses.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"

namespace pcp {
using RecSortConfig = rocprim::default_config;

// rocPRIM's radix sort in one step: the size query, the sort's temporary (a block of `tmp`,
// returned through *mem for a caller that frees it early) and the sort, on ctx's stream.  The
// iterators go to rocPRIM as they come, so a call instantiates what the two-call form did.
template <class Config = rocprim::default_config, class KI, class KO, class VI, class VO>
int sort_pairs(Tmp& tmp, KI kin, KO kout, VI vin, VO vout, size_t n, unsigned bit0, unsigned bit1,
               void** mem = nullptr) {
    pcp_ctx* ctx = tmp.ctx;
    size_t bytes = 0;
    char* m = nullptr;
    PCP_HIP(ctx, rocprim::radix_sort_pairs<Config>(nullptr, bytes, kin, kout, vin, vout, n, bit0, bit1, ctx->stream));
    PCP_TRY(tmp.get(&m, bytes));
    if (mem) *mem = m;
    PCP_HIP(ctx, rocprim::radix_sort_pairs<Config>(m, bytes, kin, kout, vin, vout, n, bit0, bit1, ctx->stream));
    return PCP_OK;
}
template <class Config = rocprim::default_config, class KI, class KO>
int sort_keys(Tmp& tmp, KI kin, KO kout, size_t n, unsigned bit0, unsigned bit1) {
    pcp_ctx* ctx = tmp.ctx;
    size_t bytes = 0;
    char* m = nullptr;
    PCP_HIP(ctx, rocprim::radix_sort_keys<Config>(nullptr, bytes, kin, kout, n, bit0, bit1, ctx->stream));
    PCP_TRY(tmp.get(&m, bytes));
    PCP_HIP(ctx, rocprim::radix_sort_keys<Config>(m, bytes, kin, kout, n, bit0, bit1, ctx->stream));
    return PCP_OK;
}
}  // namespace pcp
