// moe_entry.cuh -- the decode table's entries as the batch (moe_rows.hip) and prefill (moe_panel.hip) kernels read them.
#pragma once
#include "common.cuh"

namespace gptq {
namespace moerows {

struct Entry {                                  // one (projection, expert) of the decode table (moe_decode.hip fills it): [3 projections][E], 32 bytes
    const unsigned* tq;                         // qweight_tiled
    const void* cst;                            // qconst_tiled
    const int* perm;                            // NULL: sequential groups
    const void* reserved;
};

typedef unsigned u32x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ Entry load_entry(const Entry* p) {      // every lane loads the same 32 bytes; readfirstlane makes the pointers scalars
    const u32x8 v = *(const u32x8*)p;
    u32x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = __builtin_amdgcn_readfirstlane(v[i]);
    return __builtin_bit_cast(Entry, o);
}

}  // namespace moerows
}  // namespace gptq
