// String-producing functions over a device string column (lower, upper, slice, strip, pad,
// repeat, cat, replace; the per-row pairs out_len / write are str_dev.hpp).
//
// The output's size depends on every row, so a transform is two calls, like the gather
// (vh_str_take_plan / vh_str_take).  The plan: a length kernel writes each row's result length,
// the exclusive scan of str_col.hpp turns them into positions pos[0 .. n] in HBM, and the total
// comes back so that the caller sizes the output.  The write: every row's bytes to
// out_bytes[pos[i] ..) and the output offsets at the caller's width.
//
// The op is a template argument of both kernels: nothing is dispatched per row.  Constants
// (pattern, replacement, the cat constant) and the case table come from the host, are uploaded
// when they change and staged in LDS by every workgroup, as k_str_match stages its pattern.
// Every op runs lane per row.  The copying ops (slice, strip, pad, repeat, cat) also have the
// wave-per-row write of k_take_copy<wave>, behind the same switch (wave_form over the output's
// mean length): every lane of the wave finds the row's pieces, then takes every 64th byte of each.
// No lane waits for another, no spin loop, and no atomics outside rocPRIM's scan.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "str_col.hpp"

namespace vh {

using str::FnParams;

// LDS of an op's constants, in 8-byte words: the case table, or the constant(s)
template <int OP> constexpr uint32_t fn_lds_words() {
    return (OP == str::TF_LOWER || OP == str::TF_UPPER) ? str::FN_MAX_TABLE
           : OP == str::TF_REPLACE                      ? 2 * (STR_MAX_PATTERN / 8)
           : OP == str::TF_CAT                          ? STR_MAX_PATTERN / 8
                                                        : 1;
}

// P with its constants' pointers moved from HBM into the workgroup's LDS copy (ends in a barrier)
template <int OP> __device__ __forceinline__ FnParams stage_constants(const FnParams &P, uint64_t *lds) {
    FnParams L = P;
    if constexpr (OP == str::TF_LOWER || OP == str::TF_UPPER) {
        for (uint32_t k = threadIdx.x; k < P.ntable; k += 256) lds[k] = reinterpret_cast<const uint64_t *>(P.table)[k];
        L.table = reinterpret_cast<const uint32_t *>(lds);
        __syncthreads();
    } else if constexpr (OP == str::TF_REPLACE || OP == str::TF_CAT) {
        uint8_t *b = reinterpret_cast<uint8_t *>(lds);
        for (uint32_t k = threadIdx.x; k < P.n0; k += 256) b[k] = P.c0[k];
        L.c0 = b;
        if constexpr (OP == str::TF_REPLACE) {
            for (uint32_t k = threadIdx.x; k < P.n1; k += 256) b[STR_MAX_PATTERN + k] = P.c1[k];
            L.c1 = b + STR_MAX_PATTERN;
        }
        __syncthreads();
    }
    return L;
}

// lens[i] = bytes of row i's result, lens[n] = 0.  c2: the second column of a column cat.
// A result longer than cap (a saturated one too: repeats and widths are any int64) counts 0
// bytes and raises *too_long (every writer stores the same 1): the host keeps cap * (n + 1)
// below 2^62, so the scan's sum cannot wrap, and refuses the plan.
template <int OP>
__global__ __launch_bounds__(256) void k_fn_len(StrCol c, StrCol c2, uint64_t n, FnParams P, uint64_t cap, uint64_t *lens,
                                                uint32_t *too_long) {
    __shared__ uint64_t s_const[fn_lds_words<OP>()];
    const FnParams L = stage_constants<OP>(P, s_const);
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256) {
        uint64_t out = 0;
        if (i < n) {
            const uint8_t *p, *q = nullptr;
            uint64_t len, qlen = 0;
            row_range(c, i, p, len);
            if (OP == str::TF_CAT && (L.flags & str::FN_SECOND_COLUMN)) row_range(c2, i, q, qlen);
            out = str::out_len<OP>(L, p, len, q, qlen);
            if (out > cap) {
                out = 0;
                *too_long = 1;
            }
        }
        lens[i] = out;
    }
}

// row i's result to out_bytes[pos[i] ..) and out offsets [i] = pos[i] (i <= n; the last by the
// unit of row 0)
template <int OP, bool WAVE>
__global__ __launch_bounds__(256) void k_fn_write(StrCol c, StrCol c2, uint64_t n, FnParams P, const uint64_t *pos,
                                                  uint8_t *out_bytes, void *out_off, int out_wide) {
    __shared__ uint64_t s_const[fn_lds_words<OP>()];
    const FnParams L = stage_constants<OP>(P, s_const);
    for (uint64_t i = unit_id<WAVE>(); i < n; i += unit_stride<WAVE>()) {
        const uint64_t at = pos[i];
        if (unit_leader<WAVE>()) {
            put_offset(out_off, out_wide, i, at);
            if (i == 0) put_offset(out_off, out_wide, n, pos[n]);
        }
        const uint8_t *p, *q = nullptr;
        uint64_t len, qlen = 0;
        row_range(c, i, p, len);
        if (OP == str::TF_CAT && (L.flags & str::FN_SECOND_COLUMN)) row_range(c2, i, q, qlen);
        if constexpr (WAVE) {
            static_assert(str::is_copy_transform(OP), "the wave-per-row write is a copy of byte ranges");
            const str::Pieces s = str::pieces<OP>(L, p, len, q, qlen);
            str::pieces_write<64>(s, p, out_bytes + at, threadIdx.x & 63);  // pos[i + 1] - pos[i] bytes: the plan ran pieces too
        } else {
            str::write<OP>(L, p, len, q, qlen, out_bytes + at);
        }
    }
}

// The host's constants in HBM, one set per host thread for both calls of a pair: an upload (and
// its synchronise) is skipped while a buffer already holds the same bytes, so the write call
// and a repeated transform upload nothing.  `too_long` is the plan's flag word.
struct FnConstants {
    DevBuf c0, c1, table, too_long;
    std::vector<uint8_t> c0_host, c1_host;
    std::vector<uint32_t> table_host;  // the case table changes once per process at most
    bool c0_set = false, c1_set = false;
};
static FnConstants &fn_constants() {
    thread_local FnConstants k;
    return k;
}
// true when bytes were enqueued: the caller's buffer may go after the call, so it synchronises
static bool upload(DevBuf &dev, std::vector<uint8_t> &host, bool &set, const uint8_t *src, uint64_t n) {
    if (set && host.size() == n && (!n || !std::memcmp(host.data(), src, n))) return false;
    dev.ensure(STR_MAX_PATTERN);
    set = false;  // stays unset if the copy fails
    if (n) VH_HIP(hipMemcpyAsync(dev.ptr, src, n, hipMemcpyHostToDevice, stream()));
    host.assign(src, src + n);
    set = true;
    return n != 0;
}

static FnParams fn_params(int op, int64_t a, int64_t b, int flags, const uint8_t *c0, uint64_t n0, const uint8_t *c1,
                          uint64_t n1, const uint32_t *table, uint64_t ntable, bool second, FnConstants &k) {
    if (op < 0 || op >= str::N_TRANSFORMS) fail(VH_ERR_ARG, "vh_str_fn: unknown op");
    if (n0 > (uint64_t)STR_MAX_PATTERN || n1 > (uint64_t)STR_MAX_PATTERN) fail(VH_ERR_ARG, "vh_str_fn: a constant holds at most 1024 bytes");
    if (ntable > str::FN_MAX_TABLE) fail(VH_ERR_ARG, "vh_str_fn: a case table holds at most 2048 pairs");
    FnParams P{};
    P.a = a, P.b = b, P.flags = flags;
    hipStream_t st = stream();
    bool copied = false;
    switch (op) {
    case str::TF_LOWER:
    case str::TF_UPPER:
        if (!(flags & str::FN_ASCII) && ntable) {
            for (uint64_t i = 0; i < ntable; i++)
                if (table[2 * i] < 0x80 || (i && table[2 * i] <= table[2 * i - 2]))
                    fail(VH_ERR_ARG, "vh_str_fn: the case table is sorted by code point and holds none below 128");
            if (k.table_host.size() != 2 * ntable || std::memcmp(k.table_host.data(), table, 8 * ntable)) {
                k.table.ensure(8 * (uint64_t)str::FN_MAX_TABLE);
                VH_HIP(hipMemcpyAsync(k.table.ptr, table, 8 * ntable, hipMemcpyHostToDevice, st));
                VH_HIP(hipStreamSynchronize(st));
                k.table_host.assign(table, table + 2 * ntable);
            }
            P.table = k.table.as<uint32_t>();
            P.ntable = (uint32_t)ntable;
        }
        break;
    case str::TF_SLICE:
        if (flags & ~str::FN_HAS_STOP) fail(VH_ERR_ARG, "vh_str_fn: slice flags");
        break;
    case str::TF_STRIP:
        if (flags < str::SIDE_LEFT || flags > str::SIDE_BOTH) fail(VH_ERR_ARG, "vh_str_fn: strip side");
        for (uint64_t i = 0; i < n0; i++) {
            if (c0[i] >= 128) fail(VH_ERR_ARG, "vh_str_fn: strip takes a set of ASCII bytes");
            P.set[c0[i] >> 6] |= 1ULL << (c0[i] & 63);
        }
        break;
    case str::TF_PAD:
        if (flags < str::SIDE_LEFT || flags > str::SIDE_BOTH) fail(VH_ERR_ARG, "vh_str_fn: pad side");
        if (n0 != 1 || c0[0] >= 128) fail(VH_ERR_ARG, "vh_str_fn: the fill character is one ASCII byte");
        P.fill = c0[0];
        break;
    case str::TF_REPEAT: break;
    case str::TF_CAT:
        if (second != bool(flags & str::FN_SECOND_COLUMN)) fail(VH_ERR_ARG, "vh_str_fn: cat takes a constant or a second column");
        if (second) break;
        [[fallthrough]];
    case str::TF_REPLACE:
        if (op == str::TF_REPLACE && !n0) fail(VH_ERR_ARG, "vh_str_fn: replace takes a pattern that is not empty");
        copied = upload(k.c0, k.c0_host, k.c0_set, c0, n0);
        if (op == str::TF_REPLACE) copied |= upload(k.c1, k.c1_host, k.c1_set, c1, n1);
        if (copied) VH_HIP(hipStreamSynchronize(st));
        P.c0 = k.c0.as<uint8_t>(), P.n0 = (uint32_t)n0;
        if (op == str::TF_REPLACE) P.c1 = k.c1.as<uint8_t>(), P.n1 = (uint32_t)n1;
        break;
    }
    if (second && op != str::TF_CAT) fail(VH_ERR_ARG, "vh_str_fn: only cat takes a second column");
    return P;
}

template <int OP>
static void launch_len(const StrCol &c, const StrCol &c2, uint64_t n, const FnParams &P, uint64_t cap, uint64_t *lens,
                       uint32_t *too_long) {
    hipLaunchKernelGGL(k_fn_len<OP>, dim3(blocks_for(n + 1, 256, 16)), dim3(256), 0, stream(), c, c2, n, P, cap, lens, too_long);
}
template <int OP>
static void launch_write(bool wave, const StrCol &c, const StrCol &c2, uint64_t n, const FnParams &P, const uint64_t *pos,
                         uint8_t *out_bytes, void *out_off, int out_wide) {
    if constexpr (str::is_copy_transform(OP)) {
        if (wave) {
            hipLaunchKernelGGL((k_fn_write<OP, true>), dim3(unit_blocks<true>(n)), dim3(256), 0, stream(), c, c2, n, P, pos,
                               out_bytes, out_off, out_wide);
            return;
        }
    }
    hipLaunchKernelGGL((k_fn_write<OP, false>), dim3(unit_blocks<false>(n)), dim3(256), 0, stream(), c, c2, n, P, pos,
                       out_bytes, out_off, out_wide);
}

#define VH_FN_DISPATCH(op, call)                              \
    switch (op) {                                             \
    case str::TF_LOWER: call(str::TF_LOWER); break;           \
    case str::TF_UPPER: call(str::TF_UPPER); break;           \
    case str::TF_SLICE: call(str::TF_SLICE); break;           \
    case str::TF_STRIP: call(str::TF_STRIP); break;           \
    case str::TF_PAD: call(str::TF_PAD); break;               \
    case str::TF_REPEAT: call(str::TF_REPEAT); break;         \
    case str::TF_CAT: call(str::TF_CAT); break;               \
    default: call(str::TF_REPLACE); break;                    \
    }

}  // namespace vh

using namespace vh;

extern "C" {

int vh_str_fn_plan(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *offsets2,
                   int off2_itemsize, const uint8_t *bytes2, int op, int64_t a, int64_t b, int flags, const uint8_t *c0,
                   uint64_t n0, const uint8_t *c1, uint64_t n1, const uint32_t *table, uint64_t ntable, uint64_t *pos,
                   uint64_t *total) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    const StrCol c2 = offsets2 ? make_col(offsets2, off2_itemsize, bytes2) : StrCol{nullptr, nullptr, 0};
    FnConstants &consts = fn_constants();
    LenScratch &scratch = plan_scratch();
    const FnParams P = fn_params(op, a, b, flags, c0, n0, c1, n1, table, ntable, offsets2 != nullptr, consts);
    TimedScope ts("str_fn_plan");
    uint64_t *lens = scratch.lengths(n);
    consts.too_long.ensure(8);
    uint32_t *too_long = consts.too_long.as<uint32_t>();
    VH_HIP(hipMemsetAsync(too_long, 0, 4, stream()));
    const uint64_t cap = (1ULL << 62) / (n + 1);
#define VH_FN_LEN(OP) launch_len<OP>(c, c2, n, P, cap, lens, too_long)
    VH_FN_DISPATCH(op, VH_FN_LEN)
#undef VH_FN_LEN
    VH_HIP(hipGetLastError());
    *total = scan_lengths(scratch, n, pos);  // synchronises
    uint32_t flag = 0;
    VH_HIP(hipMemcpyAsync(&flag, too_long, 4, hipMemcpyDeviceToHost, stream()));
    VH_HIP(hipStreamSynchronize(stream()));
    if (flag) *total = VH_STR_FN_TOO_LONG;
    VH_API_END
}

int vh_str_fn(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *offsets2, int off2_itemsize,
              const uint8_t *bytes2, int op, int64_t a, int64_t b, int flags, const uint8_t *c0, uint64_t n0,
              const uint8_t *c1, uint64_t n1, const uint32_t *table, uint64_t ntable, const uint64_t *pos, uint64_t total,
              void *out_offsets, int out_itemsize, uint8_t *out_bytes) {
    VH_API_BEGIN
    const StrCol c = make_col(offsets, off_itemsize, bytes);
    const StrCol c2 = offsets2 ? make_col(offsets2, off2_itemsize, bytes2) : StrCol{nullptr, nullptr, 0};
    if (out_itemsize != 4 && out_itemsize != 8) fail(VH_ERR_ARG, "vh_str_fn: output offsets are int32 or int64");
    if (out_itemsize == 4 && str::take_needs_wide(false, total)) fail(VH_ERR_ARG, "vh_str_fn: int32 offsets overflow");
    if (total >= (1ULL << 62)) fail(VH_ERR_ARG, "vh_str_fn: the plan found the result too long");
    const FnParams P = fn_params(op, a, b, flags, c0, n0, c1, n1, table, ntable, offsets2 != nullptr, fn_constants());
    if (!n) {
        VH_HIP(hipMemsetAsync(out_offsets, 0, out_itemsize, stream()));
        return VH_OK;
    }
    TimedScope ts("str_fn");
    const bool wave = wave_form(total, n);
#define VH_FN_WRITE(OP) launch_write<OP>(wave, c, c2, n, P, pos, out_bytes, out_offsets, out_itemsize == 8)
    VH_FN_DISPATCH(op, VH_FN_WRITE)
#undef VH_FN_WRITE
    VH_HIP(hipGetLastError());
    VH_API_END
}

}  // extern "C"
