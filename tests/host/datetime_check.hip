// Runs the calendar functions of csrc/datetime_dev.hpp on the CPU (tests/test_datetime_check.py
// compares them with the numpy restatement in tests/dt_np.py): the same functions the device
// kernels inline, compiled for the host.  No GPU and no HIP runtime call.
//
// stdin: one query per line, `f unit field value` (a datetime field), `t unit field value` (a
// timedelta field; total_seconds prints the float64's bits) or `c from to value` (a unit cast),
// with the units and fields as the header's enum numbers.  stdout: one integer per query.
#include <cinttypes>
#include <cstdio>

#include "datetime_dev.hpp"

int main() {
    char kind;
    int a, b;
    long long v;
    while (std::scanf(" %c %d %d %lld", &kind, &a, &b, &v) == 4) {
        if (kind == 'f') {
            if (a < 0 || a > vh::dt::U_D || b < 0 || b >= vh::dt::N_FIELDS) return 2;
            std::printf("%d\n", (int)vh::dt::dt_field_rt(b, a, (int64_t)v));
        } else if (kind == 't') {
            if (a < 0 || a > vh::dt::U_D || b < 0 || b >= vh::dt::N_TD_FIELDS) return 2;
            std::printf("%" PRId64 "\n", (int64_t)vh::dt::td_field_rt(b, a, (int64_t)v));
        } else if (kind == 'c') {
            if (a < 0 || a > vh::dt::U_Y || b < 0 || b > vh::dt::U_Y) return 2;
            std::printf("%" PRId64 "\n", vh::dt::dt_cast_rt(a, b, (int64_t)v));
        } else {
            return 2;
        }
    }
    return 0;
}
