// Host-side check of the tone meter bank's C-ABI entries that need no device:
// rfa_tone_phasor, rfa_tone_quality, the index arithmetic the meter's kernels use, and every
// argument error of rfa_tone_* that returns before any HIP call.
// Built together with rfanalyzer_amd/csrc/tone.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cmath>
#include <cstdint>
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

static void check_phasor() {
    const double pi = 3.14159265358979323846;
    for (int32_t rate : {RFA_TONE_MIN_RATE, 48000, RFA_TONE_MAX_RATE}) {
        const int64_t M = 10LL * rate;
        double c = 9.0, s = 9.0;
        CHECK(rfa_tone_phasor(rate, 0, &c, &s) == RFA_OK && c == 1.0 && s == 0.0);
        CHECK(rfa_tone_phasor(rate, M / 4, &c, &s) == RFA_OK && std::fabs(c) <= 1e-15 && s == 1.0);
        CHECK(rfa_tone_phasor(rate, M / 2, &c, &s) == RFA_OK && c == -1.0 && std::fabs(s) <= 1e-15);
        CHECK(rfa_tone_phasor(rate, M - 1, &c, &s) == RFA_OK);
        // against the angle -2 pi / M: the table's own angle, just below 2 pi, carries two roundings
        // of up to 2^-51 each (half an ulp in [4, 8)), the functions one more of 2^-53
        CHECK(std::fabs(c - std::cos(2.0 * pi / (double)M)) <= 0x1.2p-50);
        CHECK(std::fabs(s + std::sin(2.0 * pi / (double)M)) <= 0x1.2p-50);
        CHECK(c < 1.0 && s < 0.0);
        for (int64_t p = 0; p < M; p += M / 997 + 1) {
            CHECK(rfa_tone_phasor(rate, p, &c, &s) == RFA_OK);
            CHECK(std::fabs(c * c + s * s - 1.0) <= 0x1p-51);
        }
        c = s = 9.0;
        CHECK(rfa_tone_phasor(rate, -1, &c, &s) == RFA_ERR_INVALID);
        CHECK(rfa_tone_phasor(rate, M, &c, &s) == RFA_ERR_INVALID);
        CHECK(rfa_tone_phasor(rate, INT64_MAX, &c, &s) == RFA_ERR_INVALID);
        CHECK(rfa_tone_phasor(rate, INT64_MIN, &c, &s) == RFA_ERR_INVALID);
        CHECK(rfa_tone_phasor(rate, 0, nullptr, &s) == RFA_ERR_INVALID);
        CHECK(rfa_tone_phasor(rate, 0, &c, nullptr) == RFA_ERR_INVALID);
        CHECK(c == 9.0 && s == 9.0);
    }
    double c = 9.0, s = 9.0;
    for (int32_t rate : {RFA_TONE_MIN_RATE - 1, RFA_TONE_MAX_RATE + 1, 0, -48000, INT32_MIN, INT32_MAX})
        CHECK(rfa_tone_phasor(rate, 0, &c, &s) == RFA_ERR_INVALID && c == 9.0 && s == 9.0);
}

static void check_quality() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    CHECK(std::fabs(rfa_tone_quality(500.0, 0.0, 500.0, 0.0, 1000) - 1.0) <= 1e-15);    // A = 1 at the probe
    CHECK(std::fabs(rfa_tone_quality(300.0, -400.0, 500.0, 0.0, 1000) - 1.0) <= 1e-15);
    CHECK(std::fabs(rfa_tone_quality(50.0, 0.0, 500.0, 0.0, 1000) - 0.01) <= 1e-17);
    CHECK(rfa_tone_quality(0.0, 0.0, 500.0, 0.0, 1000) == 0.0);
    CHECK(rfa_tone_quality(1.0, 1.0, 4.0, 2.0, 1) == 0.0);             // a constant row: n P = S1^2
    CHECK(rfa_tone_quality(1.0, 1.0, 1.0, 2.0, 3) == 0.0);             // a denominator below zero
    CHECK(rfa_tone_quality(0.0, 0.0, 0.0, 0.0, 0) == 0.0);
    CHECK(rfa_tone_quality(1.0, 1.0, 1.0, 0.0, 0) == 0.0);
    CHECK(rfa_tone_quality(1.0, 1.0, 1.0, 0.0, -5) == 0.0);
    // a DC offset is taken out: the same AC row on 800
    CHECK(std::fabs(rfa_tone_quality(500.0, 0.0, 500.0 + 1000.0 * 800.0 * 800.0, 800.0 * 1000.0, 1000) - 1.0) <= 1e-9);
    for (double bad : {inf, -inf, nan}) {
        CHECK(std::isnan(rfa_tone_quality(bad, 0.0, 1.0, 0.0, 10)));
        CHECK(std::isnan(rfa_tone_quality(0.0, bad, 1.0, 0.0, 10)));
        CHECK(std::isnan(rfa_tone_quality(0.0, 0.0, bad, 0.0, 10)));
        CHECK(std::isnan(rfa_tone_quality(0.0, 0.0, 1.0, bad, 10)));
        CHECK(std::isnan(rfa_tone_quality(bad, bad, bad, bad, 0)));
    }
    CHECK(std::isinf(rfa_tone_quality(1e200, 0.0, 1.0, 0.0, 10)));     // finite sums, an overflow: not a detection's business
}

// p = (f10 * (base + i)) mod M in unsigned 64-bit integers, as the kernels form it, at the largest
// operands: base = M - 1 (the counter is kept modulo M), f10 = 5 * rate - 1, i up to 2^36.
static void check_index() {
    for (int32_t rate : {RFA_TONE_MIN_RATE, 48000, RFA_TONE_MAX_RATE}) {
        const unsigned long long M = 10ULL * (unsigned long long)rate;
        const unsigned long long base = M - 1;
        for (unsigned f10 : {1u, 670u, 2541u, (unsigned)(5 * rate - 1)}) {
            for (unsigned long long i : {0ULL, 1ULL, 16384ULL, M, (1ULL << 36) - 1, 1ULL << 36}) {
                const unsigned long long g = base + i;
                const unsigned long long p = ((unsigned long long)f10 * g) % M;
                // the same through the residues: (f10 mod M) * (g mod M) mod M, each factor below 2^22
                const unsigned long long want = (((unsigned long long)f10 % M) * (g % M)) % M;
                CHECK(p == want && p < M);
                CHECK((unsigned long long)f10 * g / g == f10);        // the product did not wrap
                double c = 0.0, s = 0.0;
                CHECK(rfa_tone_phasor(rate, (int64_t)p, &c, &s) == RFA_OK);
            }
            // a counter that wraps meets the phasor of the absolute sample: base + 1 = M is 0 modulo M
            CHECK(((unsigned long long)f10 * (base + 1)) % M == 0);
        }
    }
}

static void check_create_errors() {
    rfa_tone *t = reinterpret_cast<rfa_tone *>(0x1);
    CHECK(rfa_tone_create(0, 4, 48000, nullptr) == RFA_ERR_INVALID);
    for (int32_t k : {0, -1, RFA_TONE_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) {
        t = reinterpret_cast<rfa_tone *>(0x1);
        CHECK(rfa_tone_create(0, k, 48000, &t) == RFA_ERR_INVALID && t == nullptr);
    }
    for (int32_t rate : {RFA_TONE_MIN_RATE - 1, RFA_TONE_MAX_RATE + 1, 0, -1, INT32_MIN, INT32_MAX}) {
        t = reinterpret_cast<rfa_tone *>(0x1);
        CHECK(rfa_tone_create(0, 4, rate, &t) == RFA_ERR_INVALID && t == nullptr);
    }
    // valid requests: the device is looked for only now (this program runs where there is none)
    for (int32_t k : {1, 32, RFA_TONE_MAX_CHANNELS}) {
        t = reinterpret_cast<rfa_tone *>(0x1);
        const int st = rfa_tone_create(0, k, RFA_TONE_MIN_RATE, &t);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || t == nullptr);
        if (st == RFA_OK && t) CHECK(rfa_tone_destroy(t) == RFA_OK);
    }
}

static void check_null_handle() {
    CHECK(rfa_tone_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_tone_last_error(nullptr), "null handle") == 0);
    int32_t w[3] = {9, 9, 9};
    int64_t n[2] = {9, 9};
    size_t cnt[2] = {2, 2};
    float x[4] = {9.0f, 9.0f, 9.0f, 9.0f};
    double d[16];
    for (double &v : d) v = 9.0;
    void *st = nullptr;
    CHECK(rfa_tone_get_channels(nullptr, w, w + 1) == RFA_ERR_INVALID);
    CHECK(rfa_tone_get_channels(nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_probes(nullptr, 0, w) == RFA_ERR_INVALID);
    CHECK(rfa_tone_get_probes(nullptr, 0, w) == RFA_ERR_INVALID);
    CHECK(rfa_tone_break(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_tone_break(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_tone_reset(nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process(nullptr, x, 2, cnt) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process(nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_collect(nullptr, d, n) == RFA_ERR_INVALID);
    CHECK(rfa_tone_collect(nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process_host(nullptr, x, 2, cnt, d, n) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process_host(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_tone_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w[0] == 9 && w[1] == 9 && w[2] == 9 && n[0] == 9 && n[1] == 9 && d[0] == 9.0 && d[15] == 9.0 && x[0] == 9.0f);
}

// With a device (not where the test suite runs this): the argument errors of a live handle.
static void check_live_errors() {
    rfa_tone *t = nullptr;
    if (rfa_tone_create(0, 2, RFA_TONE_MIN_RATE, &t) != RFA_OK) return;
    float x[8] = {};
    double d[16];
    int64_t n[2];
    int32_t w = 0, rate = 0;
    int32_t f10[3] = {670, 0, 693};
    size_t cnt[2] = {2, 2};
    CHECK(rfa_tone_get_channels(t, &w, &rate) == RFA_OK && w == 2 && rate == RFA_TONE_MIN_RATE);
    CHECK(rfa_tone_get_channels(t, nullptr, &rate) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_probes(t, 2, f10) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_probes(t, -1, f10) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_probes(t, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_set_probes(t, 0, f10) == RFA_OK);
    int32_t bad[3] = {670, -1, 0};
    CHECK(rfa_tone_set_probes(t, 0, bad) == RFA_ERR_INVALID);
    bad[1] = 5 * RFA_TONE_MIN_RATE;
    CHECK(rfa_tone_set_probes(t, 0, bad) == RFA_ERR_INVALID);
    int32_t got[3] = {};
    CHECK(rfa_tone_get_probes(t, 0, got) == RFA_OK && got[0] == 670 && got[1] == 0 && got[2] == 693);
    CHECK(rfa_tone_get_probes(t, 2, got) == RFA_ERR_INVALID);
    CHECK(rfa_tone_break(t, 2) == RFA_ERR_INVALID);
    CHECK(rfa_tone_break(t, -2) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process(t, nullptr, 4, cnt) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process(t, x, 4, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process(t, x, 1, cnt) == RFA_ERR_INVALID);              // a count above the stride
    cnt[1] = ((size_t)1 << 36) + 1;
    CHECK(rfa_tone_process(t, x, (size_t)1 << 37, cnt) == RFA_ERR_INVALID);
    cnt[1] = 2;
    CHECK(rfa_tone_process_host(t, x, 1, cnt, d, n) == RFA_ERR_INVALID);
    CHECK(rfa_tone_process_host(t, nullptr, 4, cnt, d, n) == RFA_ERR_INVALID);
    CHECK(rfa_tone_collect(t, d, n) == RFA_OK && d[0] == 0.0 && d[15] == 0.0 && n[1] == 0);
    CHECK(rfa_tone_destroy(t) == RFA_OK);
}

int main() {
    check_phasor();
    check_quality();
    check_index();
    check_create_errors();
    check_null_handle();
    check_live_errors();
    if (failures) {
        std::fprintf(stderr, "tone_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("tone_host_check ok\n");
    return 0;
}
