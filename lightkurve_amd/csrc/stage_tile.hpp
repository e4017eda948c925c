// stage_tile.hpp — device helper shared by pixcube.hip and psfphot.hip: a tile of consecutive cadences of a pixel cube -> LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lk {

// rows x npix floats that are CONTIGUOUS in global memory -> tile[row * pitch + column]: 16-byte loads once the
// address is aligned, scalar head and tail.
__device__ __forceinline__ void stage_contiguous(const float *__restrict__ g, float *__restrict__ tile, int total, int npix,
                                                 int pitch) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
    const int head = min(total, (4 - mis) & 3);
    if (tid < head) tile[(tid / npix) * pitch + tid % npix] = g[tid];
    const int nvec = (total - head) >> 2;
    const float4 *gv = reinterpret_cast<const float4 *>(g + head);
#pragma unroll 4
    for (int v = tid; v < nvec; v += nt) {
        const float4 x = gv[v];
        const int i = head + 4 * v;
        int r = i / npix, c = i - r * npix;
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tile[r * pitch + c] = e[k];
            if (++c == npix) {
                c = 0;
                ++r;
            }
        }
    }
    const int i = head + 4 * nvec + tid;
    if (i < total) tile[(i / npix) * pitch + i % npix] = g[i];
}

}  // namespace lk
