// sx_argmin.hpp -- the reference's epsilon comparison and argmin combine tree as device code,
// shared by every .hip file that selects a pivot (sx_kernels.hip, sx_batch.hip).  Internal linkage:
// each translation unit gets its own copy.  See the head of sx_kernels.hip for the tree.
#pragma once

#include <float.h>

#include "sx_common.hpp"

namespace {

__device__ __forceinline__ int cmp_eps(double x, double y) {
    if (fabs(x - y) < SX_EPS) return 0;
    return x < y ? -1 : 1;
}

// Lane i takes lane i + OFF's value inside its 16-lane DPP row (row_shl:OFF); a lane whose
// source is past the row keeps its own value, as a CUDA shuffle past the warp's end does.
template <int OFF>
__device__ __forceinline__ int dpp_down(int x) {
    return __builtin_amdgcn_update_dpp(x, x, 0x100 + OFF, 0xF, 0xF, false);
}
template <int OFF>
__device__ __forceinline__ double dpp_down(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = dpp_down<OFF>((int)b), hi = dpp_down<OFF>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

template <int OFF>
__device__ __forceinline__ void argmin_step(double &v, int &i, double sv, int si) {
    if (cmp_eps(sv, v) < 0) {
        v = sv;
        i = si;
    }
}

// warpReduceMin (reduction.cu:10-22) on one 32-lane half of a wave64.  Every caller reads
// the result of lane 0 of the half, whose inputs at every step come from lanes inside the
// half (lanes 0..15 take 16..31, then 0..7 take 8..15, ...), so these are exactly the
// reference's combines.  The offset-16 step crosses DPP rows (a bpermute shuffle); offsets
// 8, 4, 2, 1 stay inside row 0 and use DPP row shifts (VALU, no LDS round trip).
__device__ __forceinline__ void half_argmin(double &v, int &i) {
    argmin_step<16>(v, i, __shfl_down(v, 16, 32), __shfl_down(i, 16, 32));
    argmin_step<8>(v, i, dpp_down<8>(v), dpp_down<8>(i));
    argmin_step<4>(v, i, dpp_down<4>(v), dpp_down<4>(i));
    argmin_step<2>(v, i, dpp_down<2>(v), dpp_down<2>(i));
    argmin_step<1>(v, i, dpp_down<1>(v), dpp_down<1>(i));
}

// blockReduceMin (reduction.cu:24-49) for a 512-thread block (8 waves = 16 halves).
// Result valid in thread 0.  The same tree is the reference's 1024-thread pass 2 whenever
// at most 512 partials exist: halves 16..31 of that block would hold only (DBL_MAX, -1),
// which is exactly the padding the 512-thread final stage inserts.
__device__ __forceinline__ void block_argmin512(double &v, int &i, double *s_v, int *s_i) {
    half_argmin(v, i);
    const int lane = threadIdx.x & 31;
    const int h = threadIdx.x >> 5;
    if (lane == 0) {
        s_v[h] = v;
        s_i[h] = i;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        v = (threadIdx.x < 16) ? s_v[threadIdx.x] : DBL_MAX;
        i = (threadIdx.x < 16) ? s_i[threadIdx.x] : -1;
        half_argmin(v, i);
    }
}

// Pass 2 (deviceReduceKernel<false><<<1,1024>>>, reduction.cu:239-241) over B <= 512 tile
// winners.  A partial equal to DBL_MAX is not taken (compare(DBL_MAX, DBL_MAX) == 0), so
// its index stays -1, as in the reference.
__device__ __forceinline__ void stage2_512(const TilePart *parts, int B, double &v, int &i, double *s_v,
                                           int *s_i) {
    v = DBL_MAX;
    i = -1;
    if ((int)threadIdx.x < B) {
        const double c = parts[threadIdx.x].v;
        if (cmp_eps(c, v) < 0) {
            v = c;
            i = parts[threadIdx.x].idx;
        }
    }
    block_argmin512(v, i, s_v, s_i);
}

}  // namespace
