// Missing-value masks of HBM columns (device.py DeviceMaskedArray): the Arrow validity bitmap
// (1 = valid, LSB first) to and from the byte mask the engine takes (1 = missing), and the count
// of missing rows.  One lane per 8 rows everywhere: the bit arithmetic is mask_dev.hpp's, the
// same functions tests/host/mask_check.hip compares with a naive bit loop on the CPU.
//
// k_mask_unpack: a lane reads the one or two bitmap bytes of its 8 rows and writes one 8-byte
// word; a ragged last group or a destination that is not 8-aligned goes byte by byte.
// k_mask_pack: a lane reads one 8-byte word of the mask and writes one bitmap byte; the padding
// bits of the last byte are 0.  k_mask_count: a lane counts the non-zero bytes of its words, a
// wave adds its lanes, one atomic per wave.
#include "common.hpp"
#include "mask_dev.hpp"

namespace vh {

__global__ __launch_bounds__(256) void k_mask_unpack(const uint8_t *bits, uint64_t bit_offset, uint64_t n, uint8_t *out) {
    const bool al = aligned_rows8(out, 1);
    const uint64_t groups = (n + ROWS8 - 1) / ROWS8;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256) {
        const uint64_t row = g * ROWS8;
        if (al && n - row >= ROWS8) {
            const uint64_t w = mask::expand8(mask::valid_bits8(bits, bit_offset, row, ROWS8));
            uint2 v;
            __builtin_memcpy(&v, &w, 8);
            *reinterpret_cast<uint2 *>(out + row) = v;
        } else {
            mask::unpack_group(bits, bit_offset, n, g, out);
        }
    }
}

__device__ __forceinline__ uint64_t mask_word(const uint8_t *m, uint64_t row, uint64_t n, bool al) {
    if (al && n - row >= ROWS8) {
        const uint2 v = *reinterpret_cast<const uint2 *>(m + row);
        uint64_t w;
        __builtin_memcpy(&w, &v, 8);
        return w;
    }
    return mask::load_bytes(m, row, (uint32_t)(n - row < ROWS8 ? n - row : ROWS8));
}

__global__ __launch_bounds__(256) void k_mask_pack(const uint8_t *m, uint64_t n, uint8_t *out_bits) {
    const bool al = aligned_rows8(m, 1);
    const uint64_t groups = (n + ROWS8 - 1) / ROWS8;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256) {
        const uint64_t row = g * ROWS8;
        const uint32_t cnt = (uint32_t)(n - row < ROWS8 ? n - row : ROWS8);
        out_bits[g] = (uint8_t)mask::pack8(mask_word(m, row, n, al), cnt);
    }
}

__global__ __launch_bounds__(256) void k_mask_count(const uint8_t *m, uint64_t n, unsigned long long *total) {
    const bool al = aligned_rows8(m, 1);
    const uint64_t groups = (n + ROWS8 - 1) / ROWS8;
    unsigned long long c = 0;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256)
        c += mask::count8(mask_word(m, g * ROWS8, n, al));
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, c);
}

static void device_only(const char *fn, const void *a, const void *b) {
    if (!a || !b || resolve_loc(a, VH_LOC_AUTO) != VH_LOC_DEVICE || resolve_loc(b, VH_LOC_AUTO) != VH_LOC_DEVICE)
        fail(VH_ERR_ARG, std::string(fn) + ": device buffers only");
}

}  // namespace vh

using namespace vh;

extern "C" {

int vh_mask_unpack_bits(const uint8_t *bits, uint64_t bit_offset, uint64_t n, uint8_t *out) {
    VH_API_BEGIN
    if (!n) return VH_OK;
    device_only("vh_mask_unpack_bits", bits, out);
    TimedScope ts("mask_unpack");
    hipLaunchKernelGGL(k_mask_unpack, dim3(blocks_for((n + ROWS8 - 1) / ROWS8, 256)), dim3(256), 0, stream(), bits, bit_offset, n, out);
    VH_HIP(hipGetLastError());
    VH_API_END
}

int vh_mask_pack_bits(const uint8_t *mask, uint64_t n, uint8_t *out_bits) {
    VH_API_BEGIN
    if (!n) return VH_OK;
    device_only("vh_mask_pack_bits", mask, out_bits);
    TimedScope ts("mask_pack");
    hipLaunchKernelGGL(k_mask_pack, dim3(blocks_for((n + ROWS8 - 1) / ROWS8, 256)), dim3(256), 0, stream(), mask, n, out_bits);
    VH_HIP(hipGetLastError());
    VH_API_END
}

int vh_mask_count(const uint8_t *mask, uint64_t n, uint64_t *count) {
    VH_API_BEGIN
    if (!count) fail(VH_ERR_ARG, "vh_mask_count: null count");
    *count = 0;
    if (!n) return VH_OK;
    if (!mask || resolve_loc(mask, VH_LOC_AUTO) != VH_LOC_DEVICE) fail(VH_ERR_ARG, "vh_mask_count: device buffers only");
    hipStream_t st = stream();
    TimedScope ts("mask_count");
    DevBuf total;
    total.ensure(8);
    VH_HIP(hipMemsetAsync(total.ptr, 0, 8, st));
    hipLaunchKernelGGL(k_mask_count, dim3(blocks_for((n + ROWS8 - 1) / ROWS8, 256)), dim3(256), 0, st, mask, n,
                       total.as<unsigned long long>());
    VH_HIP(hipGetLastError());
    uint64_t host = 0;
    VH_HIP(hipMemcpyAsync(&host, total.ptr, 8, hipMemcpyDeviceToHost, st));
    VH_HIP(hipStreamSynchronize(st));
    *count = host;
    VH_API_END
}

}  // extern "C"
