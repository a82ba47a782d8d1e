// Host-side check of the frequency meter bank's C-ABI entries that need no device:
// rfa_freq_error_hz, and every argument error of rfa_freq_* that returns before any HIP call.
// Built together with rfanalyzer_amd/csrc/freq.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/rfa.h"

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static bool near(double got, double want) { return std::fabs(got - want) <= 1e-12 * std::fabs(want); }

static void check_error_hz() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double pi = 3.14159265358979323846;
    CHECK(rfa_freq_error_hz(0.0, 0.0, 96000.0) == 0.0);
    CHECK(rfa_freq_error_hz(-0.0, 0.0, 96000.0) == 0.0);          // atan2(0, -0) is pi: R1 = 0 reads 0
    CHECK(rfa_freq_error_hz(-0.0, -0.0, 96000.0) == 0.0);
    CHECK(rfa_freq_error_hz(3.0, 0.0, 96000.0) == 0.0);
    CHECK(near(rfa_freq_error_hz(0.0, 2.0, 96000.0), 24000.0));   // a quarter turn per sample
    CHECK(near(rfa_freq_error_hz(0.0, -2.0, 96000.0), -24000.0));
    CHECK(near(rfa_freq_error_hz(-1.0, 0.0, 96000.0), 48000.0));
    CHECK(near(rfa_freq_error_hz(5e-324, 5e-324, 8.0), 1.0));     // the scale of R1 does not matter
    CHECK(near(rfa_freq_error_hz(1e300, 1e300, 8.0), 1.0));
    for (double bad : {inf, -inf, nan}) {
        CHECK(std::isnan(rfa_freq_error_hz(bad, 1.0, 96000.0)));
        CHECK(std::isnan(rfa_freq_error_hz(1.0, bad, 96000.0)));
        CHECK(std::isnan(rfa_freq_error_hz(bad, bad, 96000.0)));
        CHECK(std::isnan(rfa_freq_error_hz(bad, 0.0, 96000.0)));
    }
    for (int f = -47000; f <= 47000; f += 1375) {
        const double th = 2.0 * pi * f / 96000.0;
        const double got = rfa_freq_error_hz(7.5 * std::cos(th), 7.5 * std::sin(th), 96000.0);
        CHECK(std::fabs(got - f) <= 1e-9);
    }
}

static void check_create_errors() {
    rfa_freq *f = reinterpret_cast<rfa_freq *>(0x1);
    CHECK(rfa_freq_create(0, 4, nullptr) == RFA_ERR_INVALID);
    for (int32_t k : {0, -1, RFA_FREQ_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) {
        f = reinterpret_cast<rfa_freq *>(0x1);
        CHECK(rfa_freq_create(0, k, &f) == RFA_ERR_INVALID && f == nullptr);
    }
    // valid requests: the device is looked for only now (this program runs where there is none)
    for (int32_t k : {1, 32, RFA_FREQ_MAX_CHANNELS}) {
        f = reinterpret_cast<rfa_freq *>(0x1);
        const int st = rfa_freq_create(0, k, &f);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || f == nullptr);
        if (st == RFA_OK && f) CHECK(rfa_freq_destroy(f) == RFA_OK);
    }
}

static void check_null_handle() {
    CHECK(rfa_freq_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_freq_last_error(nullptr), "null handle") == 0);
    int32_t w[2] = {9, 9};
    int64_t t[2] = {9, 9};
    float x[2] = {9.0f, 9.0f};
    double d[2] = {9.0, 9.0};
    void *st = nullptr;
    CHECK(rfa_freq_get_channels(nullptr, w) == RFA_ERR_INVALID);
    CHECK(rfa_freq_get_channels(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_break(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_freq_break(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_freq_reset(nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process(nullptr, x, x, 2, 2) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process(nullptr, nullptr, nullptr, 0, 0) == RFA_ERR_INVALID);
    CHECK(rfa_freq_collect(nullptr, d, d, t) == RFA_ERR_INVALID);
    CHECK(rfa_freq_collect(nullptr, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process_host(nullptr, x, x, 2, 2, d, d, t) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process_host(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_freq_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w[0] == 9 && w[1] == 9 && t[0] == 9 && t[1] == 9 && d[0] == 9.0 && d[1] == 9.0 && x[0] == 9.0f);
}

// With a device (not where the test suite runs this): the argument errors of a live handle.
static void check_live_errors() {
    rfa_freq *f = nullptr;
    if (rfa_freq_create(0, 3, &f) != RFA_OK) return;
    float x[8] = {};
    double d[3];
    int64_t t[3];
    int32_t w = 0;
    CHECK(rfa_freq_get_channels(f, &w) == RFA_OK && w == 3);
    CHECK(rfa_freq_get_channels(f, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_freq_break(f, 3) == RFA_ERR_INVALID);
    CHECK(rfa_freq_break(f, -2) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process(f, nullptr, x, 4, 2) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process(f, x, nullptr, 4, 2) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process(f, x, x, 1, 2) == RFA_ERR_INVALID);             // rows that overlap
    CHECK(rfa_freq_process(f, x, x, 4, (size_t)1 << 37) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process_host(f, x, x, 1, 2, d, d, t) == RFA_ERR_INVALID);
    CHECK(rfa_freq_process_host(f, nullptr, x, 4, 2, d, d, t) == RFA_ERR_INVALID);
    CHECK(rfa_freq_collect(f, d, d, t) == RFA_OK && d[0] == 0.0 && t[2] == 0);
    CHECK(rfa_freq_destroy(f) == RFA_OK);
}

int main() {
    check_error_hz();
    check_create_errors();
    check_null_handle();
    check_live_errors();
    if (failures) {
        std::fprintf(stderr, "freq_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("freq_host_check ok\n");
    return 0;
}
