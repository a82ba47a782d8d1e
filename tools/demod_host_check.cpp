// Host-side check of the demodulator's C-ABI entries that need no device: the
// mode table, the band-pass design and every error path that returns before any
// HIP call.  Built together with rfanalyzer_amd/csrc/demod.hip with the host
// compiled under AddressSanitizer and UBSan (tools/Makefile) and run as an
// ordinary program; exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/rfa.h"

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static void check_mode_table() {
    static const int32_t want[7][4] = {{96000, 0, 50000, 0},        {96000, 3000, 15000, 8000},
                                       {96000, 3000, 15000, 10000}, {384000, 30000, 150000, 100000},
                                       {96000, 1500, 5000, 2800},   {96000, 1500, 5000, 2800},
                                       {48000, 150, 800, 300}};
    for (int m = RFA_DEMOD_OFF; m <= RFA_DEMOD_CW; m++) {
        int32_t r = -1, lo = -1, hi = -1, def = -1;
        CHECK(rfa_demod_mode_info(m, &r, &lo, &hi, &def) == RFA_OK);
        CHECK(r == want[m][0] && lo == want[m][1] && hi == want[m][2] && def == want[m][3]);
        CHECK(rfa_demod_mode_info(m, nullptr, nullptr, nullptr, nullptr) == RFA_OK);
    }
    int32_t r = 0;
    CHECK(rfa_demod_mode_info(-1, &r, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_mode_info(7, &r, nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
}

static void check_band_pass(float fs, float lo, float hi) {
    int32_t n = 0;
    CHECK(rfa_bandpass_taps(1.0f, fs, lo, hi, fs * 0.01f, 40.0f, nullptr, nullptr, 0, &n) == RFA_OK);
    CHECK(n == 181);
    std::vector<float> re(n), im(n);
    // one short: nothing may be written past the capacity
    CHECK(rfa_bandpass_taps(1.0f, fs, lo, hi, fs * 0.01f, 40.0f, re.data(), im.data(), (size_t)n - 1, &n) ==
          RFA_ERR_SIZE);
    CHECK(rfa_bandpass_taps(1.0f, fs, lo, hi, fs * 0.01f, 40.0f, re.data(), im.data(), (size_t)n, &n) == RFA_OK);
    CHECK(rfa_bandpass_taps(1.0f, fs, lo, hi, fs * 0.01f, 40.0f, re.data(), nullptr, (size_t)n, &n) == RFA_OK);
    // unit gain at the centre of the pass band
    const double fc = 0.5 * ((double)lo + (double)hi);
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < n; k++) {
        const double ph = -2.0 * M_PI * fc * k / fs;
        sr += re[k] * std::cos(ph) - im[k] * std::sin(ph);
        si += re[k] * std::sin(ph) + im[k] * std::cos(ph);
    }
    CHECK(std::fabs(std::hypot(sr, si) - 1.0) < 1e-3);
}

static void check_band_pass_errors() {
    int32_t n = 5;
    float x[4];
    CHECK(rfa_bandpass_taps(1, 96000, 200, 200, 960, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID && n == 0);
    CHECK(rfa_bandpass_taps(1, 96000, 300, 200, 960, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 96000, -48001, 200, 960, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 96000, 200, 48001, 960, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 96000, 200, 2800, 0, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 96000, 200, 2800, -1, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 0, 200, 2800, 960, 40, nullptr, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_bandpass_taps(1, 96000, 200, 2800, 960, 40, x, x, 4, nullptr) == RFA_ERR_INVALID);
    // the band edges themselves are allowed
    CHECK(rfa_bandpass_taps(1, 96000, -48000, 48000, 960, 40, nullptr, nullptr, 0, &n) == RFA_OK && n == 181);
}

static void check_handle_errors() {
    rfa_demod *d = reinterpret_cast<rfa_demod *>(0x1);
    CHECK(rfa_demod_create(0, -1, &d) == RFA_ERR_INVALID && d == nullptr);   // bad mode: before any HIP call
    d = reinterpret_cast<rfa_demod *>(0x1);
    CHECK(rfa_demod_create(0, 7, &d) == RFA_ERR_INVALID && d == nullptr);
    CHECK(rfa_demod_create(0, RFA_DEMOD_AM, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_demod_last_error(nullptr), "null handle") == 0);
    int32_t w = 0;
    size_t n = 0;
    float f = 0;
    void *s = nullptr;
    CHECK(rfa_demod_set_mode(nullptr, RFA_DEMOD_AM) == RFA_ERR_INVALID);
    CHECK(rfa_demod_get_mode(nullptr, &w) == RFA_ERR_INVALID);
    CHECK(rfa_demod_set_channel_width(nullptr, 1) == RFA_ERR_INVALID);
    CHECK(rfa_demod_get_channel_width(nullptr, &w) == RFA_ERR_INVALID);
    CHECK(rfa_demod_set_volume(nullptr, 1.0f) == RFA_ERR_INVALID);
    CHECK(rfa_demod_set_audio_sink(nullptr, 1) == RFA_ERR_INVALID);
    CHECK(rfa_demod_process(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_process_host(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_max_outputs(nullptr, 1, &n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_get_taps(nullptr, 0, nullptr, nullptr, 0, &w, &w) == RFA_ERR_INVALID);
    CHECK(rfa_demod_get_state(nullptr, &f, &f, &f) == RFA_ERR_INVALID);
    CHECK(rfa_demod_reset(nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_get_stream(nullptr, &s) == RFA_ERR_INVALID);
    CHECK(rfa_demod_synchronize(nullptr) == RFA_ERR_INVALID);
}

// The bank's device-less paths: every entry on a null handle or with null outputs,
// and the creation arguments that must be rejected before the device is looked for.
static void check_bank_errors() {
    const int32_t ok_modes[3] = {RFA_DEMOD_AM, RFA_DEMOD_NFM, RFA_DEMOD_OFF};
    const int32_t bad_modes[3] = {RFA_DEMOD_AM, 7, RFA_DEMOD_NFM};
    const int32_t neg_modes[2] = {RFA_DEMOD_CW, -1};
    std::vector<int32_t> many(RFA_DEMOD_BANK_MAX_CHANNELS + 1, RFA_DEMOD_NFM);
    rfa_demod_bank *b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, ok_modes, 3, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_create(0, nullptr, 3, &b) == RFA_ERR_INVALID && b == nullptr);
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, ok_modes, 0, &b) == RFA_ERR_INVALID && b == nullptr);
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, ok_modes, -1, &b) == RFA_ERR_INVALID && b == nullptr);
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, many.data(), RFA_DEMOD_BANK_MAX_CHANNELS + 1, &b) == RFA_ERR_INVALID && b == nullptr);
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, bad_modes, 3, &b) == RFA_ERR_INVALID && b == nullptr);
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    CHECK(rfa_demod_bank_create(0, neg_modes, 2, &b) == RFA_ERR_INVALID && b == nullptr);
    // a valid request: the device is looked for only now (this program runs where there is none)
    b = reinterpret_cast<rfa_demod_bank *>(0x1);
    const int st = rfa_demod_bank_create(0, many.data(), RFA_DEMOD_BANK_MAX_CHANNELS, &b);
    CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
    CHECK((st == RFA_OK) == (b != nullptr));
    if (b) CHECK(rfa_demod_bank_destroy(b) == RFA_OK);

    CHECK(rfa_demod_bank_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_demod_bank_last_error(nullptr), "null handle") == 0);
    int32_t w = 0;
    size_t n[4] = {9, 9, 9, 9};
    float f = 0;
    void *s = nullptr;
    for (int32_t k : {0, -1, 5, RFA_DEMOD_BANK_MAX_CHANNELS}) {      // a slot index, in or out of range, on a null handle
        CHECK(rfa_demod_bank_set_mode(nullptr, k, RFA_DEMOD_AM) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_mode(nullptr, k, &w) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_mode(nullptr, k, nullptr) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_set_channel_width(nullptr, k, 1) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_channel_width(nullptr, k, &w) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_channel_width(nullptr, k, nullptr) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_set_volume(nullptr, k, 1.0f) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_set_audio_sink(nullptr, k, 1) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_taps(nullptr, k, 0, nullptr, nullptr, 0, &w, &w) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_get_state(nullptr, k, &f, &f, &f) == RFA_ERR_INVALID);
        CHECK(rfa_demod_bank_reset(nullptr, k) == RFA_ERR_INVALID);
    }
    CHECK(rfa_demod_bank_get_channels(nullptr, &w) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_get_channels(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_max_outputs(nullptr, 1, n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_max_outputs(nullptr, 1, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_process(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_process(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_process_host(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, n) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_process_host(nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(n[0] == 9 && n[3] == 9);                                    // nothing written through a null handle
    CHECK(rfa_demod_bank_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_get_stream(nullptr, &s) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_demod_bank_synchronize(nullptr) == RFA_ERR_INVALID);
}

int main() {
    check_mode_table();
    check_band_pass(96000.0f, 200.0f, 2800.0f);      // USB
    check_band_pass(96000.0f, -2800.0f, -200.0f);    // LSB
    check_band_pass(48000.0f, 600.0f, 900.0f);       // CW
    check_band_pass_errors();
    check_handle_errors();
    check_bank_errors();
    if (failures) {
        std::fprintf(stderr, "demod_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("demod_host_check ok\n");
    return 0;
}
