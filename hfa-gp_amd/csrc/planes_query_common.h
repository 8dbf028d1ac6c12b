// Point normalisation shared by the point query (planes_query.hip) and its backward (planes_query_bwd.hip): the backward
// recomputes the forward's taps, so both units must round a point the same way.
#pragma once
#include "common.h"

namespace hfagp {

// Point normalisation without contraction: hipcc fuses a * b + c into one FMA (and __fmul_rn / __fadd_rn are plain operators
// here), but torch rounds `samples * voxel_size + voxel_origin` and `(2 / box_warp) * coords` after every operation — and
// the grid must give the bits of the explicit path fed with that lattice.
__device__ __forceinline__ float scale_rn(float s, float v) {
#pragma clang fp contract(off)
    return s * v;
}
__device__ __forceinline__ float lattice_rn(int i, float voxel, float origin) {
#pragma clang fp contract(off)
    return (float)i * voxel + origin;
}

}  // namespace hfagp
