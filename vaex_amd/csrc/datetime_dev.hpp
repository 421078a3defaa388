// Calendar arithmetic on numpy datetime64[u] / timedelta64[u] tick counts, shared by the
// device expression kernels (expr.hip), the host check program (tests/host/datetime_check.hip)
// and, through it, the tests.
//
// A tick count is split once into (days since 1970-01-01, tick within the day) by a floor
// division with a compile-time divisor, written as a 64-bit multiply-high and one correction
// (no division instruction sequence, no loop); days fits int32 for years 0001..9999 in every
// unit, and everything after the split is 32-bit arithmetic with constant divisors.  Year /
// month / day come from days by the civil-from-days algorithm on 400-year eras, with floor
// semantics for days before the epoch.  The results equal numpy's casts and pandas 2's
// `.dt` / `.dt.isocalendar()` / timedelta accessors bit for bit (tests/dt_np.py restates them).
// Not pinned (undefined or an error in numpy / pandas): NaT, dates outside years 0001..9999,
// casts and arithmetic that overflow int64.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VH_DT_HD __host__ __device__ inline
#else
#define VH_DT_HD inline
#endif

namespace vh {
namespace dt {

// numpy's units, in the order of the compiler's table (vaex_amd/expr.py DT_UNITS)
enum Unit : int { U_NS = 0, U_US = 1, U_MS = 2, U_S = 3, U_MIN = 4, U_H = 5, U_D = 6, U_W = 7, U_MONTH = 8, U_Y = 9 };
constexpr int N_LINEAR = 8;  // ns .. W: a fixed number of nanoseconds each

enum Field : int {
    F_YEAR = 0, F_MONTH = 1, F_DAY = 2, F_DAYOFWEEK = 3, F_DAYOFYEAR = 4, F_QUARTER = 5, F_HALFYEAR = 6,
    F_HOUR = 7, F_MINUTE = 8, F_SECOND = 9, F_IS_LEAP_YEAR = 10, F_WEEKOFYEAR = 11, N_FIELDS = 12
};

enum TdField : int { TD_DAYS = 0, TD_SECONDS = 1, TD_MICROSECONDS = 2, TD_NANOSECONDS = 3, TD_TOTAL_SECONDS = 4, N_TD_FIELDS = 5 };

constexpr uint64_t NS_PER[N_LINEAR] = {1ull, 1000ull, 1000000ull, 1000000000ull, 60000000000ull, 3600000000000ull,
                                       86400000000000ull, 604800000000000ull};

// ticks of unit U (ns .. D) per day and per second (0: the unit is coarser than a second)
template <int U> struct UnitTraits {
    static_assert(U >= U_NS && U <= U_D, "a column unit: ns us ms s m h D");
    static constexpr uint64_t per_day = NS_PER[U_D] / NS_PER[U];
    static constexpr uint64_t per_second = U <= U_S ? NS_PER[U_S] / NS_PER[U] : 0;
};

VH_DT_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
    // the high word of the 128-bit product: 32-bit multiplies on the device, one mul on the host
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
}

// floor(2^64 / d) for a d that is no power of two (then it equals floor((2^64 - 1) / d))
constexpr uint64_t magic_of(uint64_t d) { return ~0ull / d; }
constexpr bool magic_ok(uint64_t d) { return d == 1 || (d & (d - 1)) != 0; }

// x / d for an unsigned x, any d >= 1 with magic_ok(d), m = magic_of(d): the estimate
// mulhi(x, m) is the quotient or one below it (x * m / 2^64 > x / d - 1 because
// m > 2^64 / d - 1 and x < 2^64), so one comparison of the remainder corrects it
VH_DT_HD uint64_t udiv_magic(uint64_t x, uint64_t d, uint64_t m, uint64_t *rem) {
    if (d == 1) {
        *rem = 0;
        return x;
    }
    uint64_t q = mulhi64(x, m);
    uint64_t r = x - q * d;
    if (r >= d) {
        q += 1;
        r -= d;
    }
    *rem = r;
    return q;
}

// floor(x / d) and the non-negative remainder for a signed x: a negative x is ~x >= 0, whose
// quotient q' gives floor(x / d) = ~q' (x = -(~x) - 1) and remainder d - 1 - r'
VH_DT_HD int64_t floordiv_magic(int64_t x, uint64_t d, uint64_t m, uint64_t *rem) {
    const uint64_t s = (uint64_t)(x >> 63);  // 0 or all ones
    uint64_t r;
    const uint64_t q = udiv_magic((uint64_t)x ^ s, d, m, &r);
    *rem = s ? d - 1 - r : r;
    return (int64_t)(q ^ s);
}

template <uint64_t D> VH_DT_HD int64_t floordiv_c(int64_t x, uint64_t *rem) {
    static_assert(magic_ok(D), "the divisor must not be a power of two above 1");
    return floordiv_magic(x, D, magic_of(D), rem);
}

VH_DT_HD int32_t floordiv32(int32_t a, int32_t b) {  // b > 0 a constant at every call site
    const int32_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

VH_DT_HD bool is_leap(int32_t y) { return (y & 3) == 0 && (y % 100 != 0 || y % 400 == 0); }

struct Civil {
    int32_t year, month, day;  // month 1..12, day 1..31
    int32_t doy;               // day of the year, 1..366
};

// days since 1970-01-01 -> proleptic Gregorian date, on 400-year eras that start on March 1
// (H. Hinnant, "chrono-Compatible Low-Level Date Algorithms", public domain)
VH_DT_HD Civil civil_from_days(int32_t days) {
    const int32_t z = days + 719468;
    const int32_t era = floordiv32(z, 146097);
    const uint32_t doe = (uint32_t)(z - era * 146097);                               // [0, 146096]
    const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;      // [0, 399]
    const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                    // [0, 365], from March 1
    const uint32_t mp = (5 * doy + 2) / 153;                                         // [0, 11], March = 0
    Civil c;
    c.day = (int32_t)(doy - (153 * mp + 2) / 5 + 1);
    c.month = (int32_t)(mp < 10 ? mp + 3 : mp - 9);
    c.year = (int32_t)yoe + era * 400 + (c.month <= 2);
    c.doy = mp < 10 ? (int32_t)doy + 60 + (is_leap(c.year) ? 1 : 0) : (int32_t)doy - 305;
    return c;
}

VH_DT_HD int32_t days_from_civil(int32_t y, int32_t m, int32_t d) {
    y -= m <= 2;
    const int32_t era = floordiv32(y, 400);
    const uint32_t yoe = (uint32_t)(y - era * 400);
    const uint32_t doy = (153 * (uint32_t)(m > 2 ? m - 3 : m + 9) + 2) / 5 + (uint32_t)d - 1;
    const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + (int32_t)doe - 719468;
}

// ticks of unit U -> (days since the epoch, tick within the day)
template <int U> VH_DT_HD int32_t split_days(int64_t x, uint64_t *tod) {
    if constexpr (U == U_D) {
        *tod = 0;
        return (int32_t)x;
    } else {
        return (int32_t)floordiv_c<UnitTraits<U>::per_day>(x, tod);
    }
}

// second of the day from the tick within the day
template <int U> VH_DT_HD uint32_t second_of_day(uint64_t tod) {
    if constexpr (U == U_NS || U == U_US) {  // tod < 86400e9: one more 64-bit multiply-high
        uint64_t r;
        return (uint32_t)udiv_magic(tod, UnitTraits<U>::per_second, magic_of(UnitTraits<U>::per_second), &r);
    } else if constexpr (U == U_MS) {
        return (uint32_t)tod / 1000u;
    } else if constexpr (U == U_S) {
        return (uint32_t)tod;
    } else if constexpr (U == U_MIN) {
        return (uint32_t)tod * 60u;
    } else if constexpr (U == U_H) {
        return (uint32_t)tod * 3600u;
    } else {
        return 0;
    }
}

// One datetime field of a tick count of unit U.  weekofyear is the ISO-8601 week (the week
// with the year's first Thursday is week 1): the week of the year of the Thursday of x's week.
template <int U, int F> VH_DT_HD int32_t dt_field(int64_t x) {
    uint64_t tod;
    const int32_t days = split_days<U>(x, &tod);
    if constexpr (F == F_HOUR || F == F_MINUTE || F == F_SECOND) {
        const uint32_t sod = second_of_day<U>(tod);
        return F == F_HOUR ? (int32_t)(sod / 3600u) : F == F_MINUTE ? (int32_t)(sod / 60u % 60u) : (int32_t)(sod % 60u);
    } else if constexpr (F == F_DAYOFWEEK || F == F_WEEKOFYEAR) {
        int32_t dow = (days + 3) % 7;  // 1970-01-01 is a Thursday; Monday = 0
        dow = dow < 0 ? dow + 7 : dow;
        if constexpr (F == F_DAYOFWEEK) return dow;
        return (civil_from_days(days - dow + 3).doy - 1) / 7 + 1;
    } else {
        const Civil c = civil_from_days(days);
        switch (F) {
        case F_YEAR: return c.year;
        case F_MONTH: return c.month;
        case F_DAY: return c.day;
        case F_DAYOFYEAR: return c.doy;
        case F_QUARTER: return (c.month - 1) / 3 + 1;
        case F_HALFYEAR: return (c.month - 1) / 6 + 1;
        default: return is_leap(c.year) ? 1 : 0;  // F_IS_LEAP_YEAR
        }
    }
}

template <int U> VH_DT_HD int32_t dt_field_u(int field, int64_t x) {
    switch (field) {
    case F_YEAR: return dt_field<U, F_YEAR>(x);
    case F_MONTH: return dt_field<U, F_MONTH>(x);
    case F_DAY: return dt_field<U, F_DAY>(x);
    case F_DAYOFWEEK: return dt_field<U, F_DAYOFWEEK>(x);
    case F_DAYOFYEAR: return dt_field<U, F_DAYOFYEAR>(x);
    case F_QUARTER: return dt_field<U, F_QUARTER>(x);
    case F_HALFYEAR: return dt_field<U, F_HALFYEAR>(x);
    case F_HOUR: return dt_field<U, F_HOUR>(x);
    case F_MINUTE: return dt_field<U, F_MINUTE>(x);
    case F_SECOND: return dt_field<U, F_SECOND>(x);
    case F_IS_LEAP_YEAR: return dt_field<U, F_IS_LEAP_YEAR>(x);
    default: return dt_field<U, F_WEEKOFYEAR>(x);
    }
}

// the same with the unit at run time (the interpreter's entry; the check program's too)
VH_DT_HD int32_t dt_field_rt(int field, int unit, int64_t x) {
    switch (unit) {
    case U_NS: return dt_field_u<U_NS>(field, x);
    case U_US: return dt_field_u<U_US>(field, x);
    case U_MS: return dt_field_u<U_MS>(field, x);
    case U_S: return dt_field_u<U_S>(field, x);
    case U_MIN: return dt_field_u<U_MIN>(field, x);
    case U_H: return dt_field_u<U_H>(field, x);
    default: return dt_field_u<U_D>(field, x);
    }
}

// Timedelta fields with pandas' definitions: days is the floor, seconds / microseconds /
// nanoseconds are the non-negative remainders (-1 ns: days -1, seconds 86399, microseconds
// 999999, nanoseconds 999).  The result is int64 bits; total_seconds is float64 bits:
// ticks / ticks-per-second in float64 below a second (pandas: asi8 / periods_per_second),
// the exact integer of seconds converted once from a second up.
template <int U> VH_DT_HD uint64_t td_field_u(int field, int64_t x) {
    if (field == TD_TOTAL_SECONDS) {
        double s;
        if constexpr (U <= U_S) s = (double)x / (double)UnitTraits<U>::per_second;
        else s = (double)(x * (int64_t)(NS_PER[U] / NS_PER[U_S]));
        return __builtin_bit_cast(uint64_t, s);
    }
    uint64_t tod;
    int64_t days;
    if constexpr (U == U_D) {
        days = x;
        tod = 0;
    } else {
        days = floordiv_c<UnitTraits<U>::per_day>(x, &tod);
    }
    if (field == TD_DAYS) return (uint64_t)days;
    if (field == TD_SECONDS) return second_of_day<U>(tod);
    // the ticks below a second, in nanoseconds (< 1e9)
    uint32_t sub = 0;
    if constexpr (U == U_NS || U == U_US) {
        uint64_t r;
        udiv_magic(tod, UnitTraits<U>::per_second, magic_of(UnitTraits<U>::per_second), &r);
        sub = (uint32_t)r * (uint32_t)NS_PER[U];
    } else if constexpr (U == U_MS) {
        sub = (uint32_t)tod % 1000u * 1000000u;
    }
    return field == TD_MICROSECONDS ? sub / 1000u : sub % 1000u;
}

VH_DT_HD uint64_t td_field_rt(int field, int unit, int64_t x) {
    switch (unit) {
    case U_NS: return td_field_u<U_NS>(field, x);
    case U_US: return td_field_u<U_US>(field, x);
    case U_MS: return td_field_u<U_MS>(field, x);
    case U_S: return td_field_u<U_S>(field, x);
    case U_MIN: return td_field_u<U_MIN>(field, x);
    case U_H: return td_field_u<U_H>(field, x);
    default: return td_field_u<U_D>(field, x);
    }
}

// ---- unit casts: astype(x, 'datetime64[to]') / 'timedelta64[to]' ------------------------
// Among ns .. W: coarser -> finer multiplies, finer -> coarser is a floor division by the
// ratio (a multiply-high with the ratio's magic number).  To M / Y through the civil date
// (numpy floors: 1969-12-31 is month -1, year -1); from M / Y through days-from-civil of the
// first of the month.  timedelta64 casts never cross the M / Y boundary (numpy refuses them;
// the compiler does too), M <-> Y is the same x12 for both kinds.
// ticks of the finer unit `to` in one tick of FROM, picked from constants (no run-time division)
template <int FROM> VH_DT_HD uint64_t ratio_up(int to) {
    switch (to) {
    case U_NS: if constexpr (FROM > U_NS) return NS_PER[FROM] / NS_PER[U_NS]; break;
    case U_US: if constexpr (FROM > U_US) return NS_PER[FROM] / NS_PER[U_US]; break;
    case U_MS: if constexpr (FROM > U_MS) return NS_PER[FROM] / NS_PER[U_MS]; break;
    case U_S: if constexpr (FROM > U_S) return NS_PER[FROM] / NS_PER[U_S]; break;
    case U_MIN: if constexpr (FROM > U_MIN) return NS_PER[FROM] / NS_PER[U_MIN]; break;
    case U_H: if constexpr (FROM > U_H) return NS_PER[FROM] / NS_PER[U_H]; break;
    case U_D: if constexpr (FROM > U_D) return NS_PER[FROM] / NS_PER[U_D]; break;
    }
    return 1;
}

VH_DT_HD uint64_t ratio_up_rt(int from, int to) {
    switch (from) {
    case U_US: return ratio_up<U_US>(to);
    case U_MS: return ratio_up<U_MS>(to);
    case U_S: return ratio_up<U_S>(to);
    case U_MIN: return ratio_up<U_MIN>(to);
    case U_H: return ratio_up<U_H>(to);
    case U_D: return ratio_up<U_D>(to);
    case U_W: return ratio_up<U_W>(to);
    }
    return 1;
}

// the ratio's magic number with the target unit at compile time, so that it is a constant
template <int TO> VH_DT_HD int64_t cast_down(int from, int64_t x) {
    uint64_t r;
    switch (from) {
    case U_NS: if constexpr (TO > U_NS) return floordiv_c<NS_PER[TO] / NS_PER[U_NS]>(x, &r); break;
    case U_US: if constexpr (TO > U_US) return floordiv_c<NS_PER[TO] / NS_PER[U_US]>(x, &r); break;
    case U_MS: if constexpr (TO > U_MS) return floordiv_c<NS_PER[TO] / NS_PER[U_MS]>(x, &r); break;
    case U_S: if constexpr (TO > U_S) return floordiv_c<NS_PER[TO] / NS_PER[U_S]>(x, &r); break;
    case U_MIN: if constexpr (TO > U_MIN) return floordiv_c<NS_PER[TO] / NS_PER[U_MIN]>(x, &r); break;
    case U_H: if constexpr (TO > U_H) return floordiv_c<NS_PER[TO] / NS_PER[U_H]>(x, &r); break;
    case U_D: if constexpr (TO > U_D) return floordiv_c<NS_PER[TO] / NS_PER[U_D]>(x, &r); break;
    }
    return x;
}

VH_DT_HD int64_t cast_linear(int from, int to, int64_t x) {
    if (from == to) return x;
    if (from > to) return (int64_t)((uint64_t)x * ratio_up_rt(from, to));
    switch (to) {  // every ratio has a factor 3, 5 or 7: none is a power of two
    case U_US: return cast_down<U_US>(from, x);
    case U_MS: return cast_down<U_MS>(from, x);
    case U_S: return cast_down<U_S>(from, x);
    case U_MIN: return cast_down<U_MIN>(from, x);
    case U_H: return cast_down<U_H>(from, x);
    case U_D: return cast_down<U_D>(from, x);
    default: return cast_down<U_W>(from, x);
    }
}

VH_DT_HD int64_t dt_cast_rt(int from, int to, int64_t x) {
    if (from < N_LINEAR && to < N_LINEAR) return cast_linear(from, to, x);
    if (from >= N_LINEAR && to >= N_LINEAR) {  // M <-> Y
        if (from == to) return x;
        if (from == U_Y) return (int64_t)((uint64_t)x * 12u);
        uint64_t r;
        return floordiv_c<12>(x, &r);
    }
    if (to >= N_LINEAR) {  // a linear unit -> months / years since 1970
        const Civil c = civil_from_days((int32_t)cast_linear(from, U_D, x));
        return to == U_Y ? (int64_t)(c.year - 1970) : (int64_t)(c.year - 1970) * 12 + (c.month - 1);
    }
    // months / years since 1970 -> the first day of that month / year
    int32_t y, m = 1;
    if (from == U_Y) {
        y = (int32_t)x + 1970;
    } else {
        uint64_t r;
        y = (int32_t)floordiv_c<12>(x, &r) + 1970;
        m = (int32_t)r + 1;
    }
    return cast_linear(U_D, to, (int64_t)days_from_civil(y, m, 1));
}

}  // namespace dt
}  // namespace vh
