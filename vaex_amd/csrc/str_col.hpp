// What the string kernels of strings.hip and strfn.hip share: the column view, the choice
// between the lane-per-row and the wave-per-row form, and the scan that turns per-row output
// lengths into positions (the plan half of every call pair whose output size depends on the
// data: vh_str_take_plan, vh_str_fn_plan).
#pragma once

#include <rocprim/device/device_scan.hpp>

#include <cstdlib>

#include "common.hpp"
#include "str_dev.hpp"

namespace vh {

constexpr int STR_MAX_PATTERN = 1024;

struct StrCol {
    const void *off;
    const uint8_t *bytes;
    int wide;  // int64 offsets
};

__device__ __forceinline__ int64_t col_off(const StrCol &c, uint64_t i) {
    return c.wide ? static_cast<const int64_t *>(c.off)[i] : (int64_t) static_cast<const int32_t *>(c.off)[i];
}
__device__ __forceinline__ void row_range(const StrCol &c, uint64_t i, const uint8_t *&p, uint64_t &len) {
    const int64_t a = col_off(c, i), e = col_off(c, i + 1);
    p = c.bytes + a;
    len = (uint64_t)(e - a);
}

static StrCol make_col(const void *off, int itemsize, const uint8_t *bytes) {
    if (itemsize != 4 && itemsize != 8) fail(VH_ERR_ARG, "string offsets are int32 or int64");
    return StrCol{off, bytes, itemsize == 8};
}

// the host's choice of form: wave per row from this mean length on (VH_STR_FORM=lane|wave pins it).
// Measured: the lane form wins up to a mean of 128 bytes, the wave form from 256.
constexpr uint64_t STR_WAVE_MEAN = 256;
static bool wave_form(uint64_t total_bytes, uint64_t rows) {
    const char *pin = std::getenv("VH_STR_FORM");  // read per call: scripts/str_bench.py flips it
    if (pin && pin[0] == 'l') return false;
    if (pin && pin[0] == 'w') return true;
    return rows && total_bytes / rows >= STR_WAVE_MEAN;
}
// bytes the rows [0, n) of a checked column span (two offsets read back)
static uint64_t col_span(const StrCol &c, uint64_t n) {
    if (!n) return 0;
    int64_t a = 0, e = 0;
    const int isz = c.wide ? 8 : 4;
    VH_HIP(hipMemcpyAsync(&a, c.off, isz, hipMemcpyDeviceToHost, stream()));
    VH_HIP(hipMemcpyAsync(&e, static_cast<const char *>(c.off) + n * isz, isz, hipMemcpyDeviceToHost, stream()));
    VH_HIP(hipStreamSynchronize(stream()));
    if (!c.wide) {
        int32_t a4, e4;
        __builtin_memcpy(&a4, &a, 4);
        __builtin_memcpy(&e4, &e, 4);
        a = a4;
        e = e4;
    }
    return e > a ? (uint64_t)(e - a) : 0;
}

// units (rows) of a launch: a lane or a wave each
template <bool WAVE> __device__ __forceinline__ uint64_t unit_id() {
    const uint64_t t = blockIdx.x * 256ull + threadIdx.x;
    return WAVE ? t >> 6 : t;
}
template <bool WAVE> __device__ __forceinline__ uint64_t unit_stride() { return (uint64_t)gridDim.x * (WAVE ? 4 : 256); }
template <bool WAVE> __device__ __forceinline__ bool unit_leader() { return !WAVE || (threadIdx.x & 63) == 0; }
template <bool WAVE> static unsigned unit_blocks(uint64_t rows) { return blocks_for(WAVE ? rows * 64 : rows, 256, 16); }

// entry k of an output column's offsets, at its width
__device__ __forceinline__ void put_offset(void *out_off, int out_wide, uint64_t k, uint64_t v) {
    if (out_wide) static_cast<int64_t *>(out_off)[k] = (int64_t)v;
    else static_cast<int32_t *>(out_off)[k] = (int32_t)v;
}

// a plan's scratch: the m + 1 lengths (the last 0) a length kernel writes, and rocPRIM's.  One
// per host thread for every plan (the gather's and the transforms': strings.hip defines it); it
// keeps 8 bytes per row of the largest column planned so far, like the library's other scratch.
struct LenScratch {
    DevBuf lens, tmp;
    uint64_t *lengths(uint64_t m) {
        lens.ensure((m + 1) * 8);
        return lens.as<uint64_t>();
    }
};
LenScratch &plan_scratch();
// pos[0 .. m] = the exclusive scan of the lengths; returns the total (pos[m]) after a sync
static uint64_t scan_lengths(LenScratch &s, uint64_t m, uint64_t *pos) {
    hipStream_t st = stream();
    size_t tb = 0;
    VH_HIP(rocprim::exclusive_scan(nullptr, tb, s.lens.as<uint64_t>(), pos, (uint64_t)0, (size_t)(m + 1),
                                   rocprim::plus<uint64_t>(), st));
    s.tmp.ensure(tb ? tb : 8);
    VH_HIP(rocprim::exclusive_scan(s.tmp.ptr, tb, s.lens.as<uint64_t>(), pos, (uint64_t)0, (size_t)(m + 1),
                                   rocprim::plus<uint64_t>(), st));
    uint64_t total = 0;
    VH_HIP(hipMemcpyAsync(&total, pos + m, 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    return total;
}

}  // namespace vh
