// Wavefront-wide sums, prefix sums and minima / maxima with DPP row shifts and row broadcasts: a handful of VALU operations where a
// __shfl_xor / __shfl_up ladder pays an LDS-crossbar permute (ds_bpermute_b32, a dependent LDS round trip) per step and 32-bit word.
// Shared by the ILP launch (mht_blp.hip) and the grow launch (mht_fgrow_dev.h).  EVERY lane of the wavefront must be active at the call.
#pragma once
#include "mht_common.h"

namespace mht {

// wave64 sum; fixed summation order -> deterministic.  Result is valid in every lane.  The order is the balanced pairwise tree over the
// lanes -- six rounds of x = x[0::2] + x[1::2], lane 63's path never meets a zero fill -- and tests/test_devprobe_gpu.py holds it to that bit for bit.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_f64<0x111, 0xf>(v);      // row_shr:1
    v += dpp_f64<0x112, 0xf>(v);      // row_shr:2
    v += dpp_f64<0x114, 0xf>(v);      // row_shr:4
    v += dpp_f64<0x118, 0xf>(v);      // row_shr:8   -> lane 15 of every row holds the row sum
    v += dpp_f64<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v += dpp_f64<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// wave64 INCLUSIVE prefix sum of a 32-bit value, the same row shifts / row broadcasts: six VALU adds where a __shfl_up scan pays an
// LDS-crossbar permute per step (two for a 64-bit value).  Lanes without a source lane add 0.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned wave_scan_u32(unsigned v) {
    v += dpp_u32<0x111, 0xf>(v);      // row_shr:1
    v += dpp_u32<0x112, 0xf>(v);      // row_shr:2
    v += dpp_u32<0x114, 0xf>(v);      // row_shr:4
    v += dpp_u32<0x118, 0xf>(v);      // row_shr:8   -> inclusive within every row of 16
    v += dpp_u32<0x142, 0xa>(v);      // row_bcast:15: the sum of row 0 into row 1, of row 2 into row 3
    v += dpp_u32<0x143, 0xc>(v);      // row_bcast:31: the sum of rows 0 and 1 into rows 2 and 3
    return v;
}
// the sum of a 32-bit value over the wavefront, in every lane (a scalar register)
__device__ __forceinline__ int wave_sum_i32(int v) { return __builtin_amdgcn_readlane((int)wave_scan_u32((unsigned)v), 63); }

// minimum / maximum of a signed 32-bit value over the wavefront, in every lane (a scalar register).  Lanes without a source lane see
// their own value again.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_self_i32(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, dpp_self_i32<0x111, 0xf>(v));
    v = min(v, dpp_self_i32<0x112, 0xf>(v));
    v = min(v, dpp_self_i32<0x114, 0xf>(v));
    v = min(v, dpp_self_i32<0x118, 0xf>(v));      // lane 15 of every row holds the row's
    v = min(v, dpp_self_i32<0x142, 0xa>(v));      // row_bcast:15
    v = min(v, dpp_self_i32<0x143, 0xc>(v));      // row_bcast:31 -> lane 63 holds the wavefront's
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_max_i32(int v) {
    v = max(v, dpp_self_i32<0x111, 0xf>(v));
    v = max(v, dpp_self_i32<0x112, 0xf>(v));
    v = max(v, dpp_self_i32<0x114, 0xf>(v));
    v = max(v, dpp_self_i32<0x118, 0xf>(v));
    v = max(v, dpp_self_i32<0x142, 0xa>(v));
    v = max(v, dpp_self_i32<0x143, 0xc>(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// minimum of a value over a 16-lane row (result in lane 15 of the row) / the wavefront (result in every lane): three VALU
// ops per step where the (value, index) pair needs a dozen
template <int CTRL, int ROW_MASK> __device__ __forceinline__ void dpp_min_value(double& v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int nlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int nhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    v = fmin(v, __hiloint2double(nhi, nlo));
}
__device__ __forceinline__ double row16_min_value(double v) {
    dpp_min_value<0x111, 0xf>(v);
    dpp_min_value<0x112, 0xf>(v);
    dpp_min_value<0x114, 0xf>(v);
    dpp_min_value<0x118, 0xf>(v);
    return v;
}
__device__ __forceinline__ double wave_min_value(double v) {
    v = row16_min_value(v);
    dpp_min_value<0x142, 0xa>(v);      // row_bcast:15
    dpp_min_value<0x143, 0xc>(v);      // row_bcast:31 -> lane 63 holds the minimum
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
// lexicographic (value, index) minimum over the wavefront with DPP (index -1 = none); result valid in every lane
template <int CTRL, int ROW_MASK> __device__ __forceinline__ void dpp_min_pair(double& v, int& i) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int nlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int nhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const int ni = __builtin_amdgcn_update_dpp(i, i, CTRL, ROW_MASK, 0xf, false);
    const double nv = __hiloint2double(nhi, nlo);
    if (ni >= 0 && (i < 0 || nv < v || (nv == v && ni < i))) { v = nv; i = ni; }
}
__device__ __forceinline__ void row16_min_pair(double& v, int& i) {      // lane 15 of every 16-lane row gets the row minimum
    dpp_min_pair<0x111, 0xf>(v, i);
    dpp_min_pair<0x112, 0xf>(v, i);
    dpp_min_pair<0x114, 0xf>(v, i);
    dpp_min_pair<0x118, 0xf>(v, i);
}
__device__ __forceinline__ void wave_min_pair(double& v, int& i) {
    row16_min_pair(v, i);
    dpp_min_pair<0x142, 0xa>(v, i);      // row_bcast:15
    dpp_min_pair<0x143, 0xc>(v, i);      // row_bcast:31 -> lane 63 holds the minimum
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63), lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    v = __hiloint2double(hi, lo);
    i = __builtin_amdgcn_readlane(i, 63);
}

}  // namespace mht
