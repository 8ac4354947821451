// Host-only check of elimrec_amd/csrc/dispatch.h (no HIP, no GPU):
//   c++ -std=c++17 -Wall -g -fsanitize=address,undefined tools/dispatch_check.cpp -o dispatch_check && ./dispatch_check
// exits 0 and prints "dispatch_check: ok", or says which expectation failed.
#include <cstdarg>
#include <cstdio>
#include <initializer_list>

static int g_raised = 0;
static const void *g_raised_fn = nullptr;
static size_t g_raised_bytes = 0;
#define ELIMREC_RAISE_LDS_LIMIT(kernel, bytes) (++g_raised, g_raised_fn = (const void *)(kernel), g_raised_bytes = (bytes))
#include "../elimrec_amd/csrc/dispatch.h"

static int g_errors = 0;
static char g_msg[256];
void elimrec::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    ++g_errors;
}

static int g_failed = 0;
#define EXPECT(cond) \
    do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

template <int MIN> static void check_pow2() {
    for (int v = -70; v <= 300; ++v) {
        const bool ok = v >= MIN && v <= 64 && (v & (v - 1)) == 0;
        for (int ret : {0, 7, ELIMREC_E_UNSUPPORTED}) {
            int calls = 0, seen = -1;
            const int errors = g_errors;
            const int rc = elimrec::with_pow2<MIN>("check", v, [&](auto c) {
                static_assert(decltype(c)::value >= MIN && decltype(c)::value <= 64, "no instantiation outside [MIN, 64]");
                ++calls;
                seen = decltype(c)::value;
                return ret;
            });
            if (ok) EXPECT(calls == 1 && seen == v && rc == ret && g_errors == errors);
            else EXPECT(calls == 0 && rc == ELIMREC_E_BADARG && g_errors == errors + 1);
        }
    }
}

static void check_quads() {
    for (int d = -70; d <= 600; ++d) {
        const bool ok = d >= 4 && d <= 256;                    // (d % 4 is the entry points' check, not the selector's)
        for (int ret : {0, 7, ELIMREC_E_UNSUPPORTED}) {
            int calls = 0, seen = -1;
            const int errors = g_errors;
            const int rc = elimrec::with_quads("check", d, [&](auto c) {
                static_assert(decltype(c)::value >= 1 && decltype(c)::value <= 4, "no instantiation outside [1, 4]");
                ++calls;
                seen = decltype(c)::value;
                return ret;
            });
            if (ok) EXPECT(calls == 1 && seen == (d + 63) / 64 && rc == ret && g_errors == errors);
            else EXPECT(calls == 0 && rc == ELIMREC_E_BADARG && g_errors == errors + 1);
        }
    }
}

static void kernel_a() {}
static void kernel_b() {}

int main() {
    check_pow2<1>();
    check_pow2<4>();
    // the cases the selector is there to refuse, by name: 0, 3, negative, 128, a power of two below MIN
    for (int v : {0, 3, -8, 128, 2}) {
        int calls = 0;
        EXPECT(elimrec::with_pow2<4>("check", v, [&](auto) { return ++calls; }) == ELIMREC_E_BADARG && calls == 0);
    }
    EXPECT(elimrec::with_pow2<1>("check", 2, [](auto c) { return 100 + decltype(c)::value; }) == 102);

    check_quads();
    // both sides of every width boundary, and the two ends, by name
    for (int d : {4, 64, 68, 128, 132, 192, 196, 256})
        EXPECT(elimrec::with_quads("check", d, [](auto c) { return 100 + decltype(c)::value; }) == 100 + (d + 63) / 64);
    for (int d : {0, 3, -4, 257, 260, 320}) {
        int calls = 0;
        EXPECT(elimrec::with_quads("check", d, [&](auto) { return ++calls; }) == ELIMREC_E_BADARG && calls == 0);
    }

    EXPECT(elimrec::with_fast(true, [](auto f) { return decltype(f)::value ? 1 : 2; }) == 1);
    EXPECT(elimrec::with_fast(false, [](auto f) { return decltype(f)::value ? 1 : 2; }) == 2);
    int fast_calls = 0;
    elimrec::with_fast(true, [&](auto) { ++fast_calls; });      // a body without a result, as the evaluator's are
    EXPECT(fast_calls == 1);

    // allow_lds: through to the HIP call once per instantiation, with the first call's size
    for (int k = 0; k < 3; ++k) elimrec::allow_lds<kernel_a>(100 * 1024 + k);
    EXPECT(g_raised == 1 && g_raised_fn == (const void *)kernel_a && g_raised_bytes == 100 * 1024);
    for (int k = 0; k < 3; ++k) elimrec::allow_lds<kernel_b>(160 * 1024);
    EXPECT(g_raised == 2 && g_raised_fn == (const void *)kernel_b && g_raised_bytes == 160 * 1024);
    elimrec::allow_lds<kernel_a>(160 * 1024);
    EXPECT(g_raised == 2);

    if (g_failed) { std::printf("dispatch_check: %d expectation(s) failed\n", g_failed); return 1; }
    std::printf("dispatch_check: ok\n");
    return 0;
}
