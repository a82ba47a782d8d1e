// Host-side check of the polyphase channelizer's C-ABI entries that need no
// device: the length rule and every error path that returns before any HIP call.
// Built together with rfanalyzer_amd/csrc/channelizer.hip with the host compiled
// under AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary
// program; exits 0 when every check holds.
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

static bool smooth(int n) {
    if (n < RFA_PFB_MIN_CHANNELS || n > RFA_PFB_MAX_CHANNELS) return false;
    for (int f : {2, 3, 5})
        while (n % f == 0) n /= f;
    return n == 1;
}

static void check_supported() {
    for (int n = -20; n <= 5000; n++) CHECK((rfa_pfb_supported(n) == 1) == smooth(n));
    CHECK(rfa_pfb_supported(INT32_MIN) == 0 && rfa_pfb_supported(INT32_MAX) == 0);
    CHECK(rfa_pfb_supported(96) == 1 && rfa_pfb_supported(100) == 1 && rfa_pfb_supported(400) == 1);
    CHECK(rfa_pfb_supported(7) == 0 && rfa_pfb_supported(14) == 0 && rfa_pfb_supported(4097) == 0);
}

static int create(int fmt, int32_t m, int32_t d, const float *taps, int32_t t, bool *null_out) {
    rfa_pfb *p = reinterpret_cast<rfa_pfb *>(0x1);
    const int st = rfa_pfb_create(0, fmt, m, d, taps, t, &p);
    *null_out = p == nullptr;
    if (st == RFA_OK && p) rfa_pfb_destroy(p);
    return st;
}

static void check_create_errors() {
    std::vector<float> taps(16 * 4096 + 1, 0.25f);
    const float *h = taps.data();
    bool nul = false;
    CHECK(rfa_pfb_create(0, RFA_IN_S8, 16, 4, h, 16, nullptr) == RFA_ERR_INVALID);
    // every invalid argument: before the device is looked for, *out cleared
    CHECK(create(-1, 16, 4, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_F32_PLANAR, 16, 4, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 0, 1, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, -16, 1, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 0, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, -3, h, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 17, h, 16, &nul) == RFA_ERR_INVALID && nul);        // decimation above n_channels
    CHECK(create(RFA_IN_S8, 16, 4, nullptr, 16, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 4, h, 0, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 4, h, -1, &nul) == RFA_ERR_INVALID && nul);
    CHECK(create(RFA_IN_S8, 16, 4, h, 16 * 16 + 1, &nul) == RFA_ERR_INVALID && nul);  // more than 16 phases
    CHECK(create(RFA_IN_S8, 4096, 4, h, 16 * 4096 + 1, &nul) == RFA_ERR_INVALID && nul);
    // a length the DFT does not take: unsupported, after the invalid arguments
    for (int32_t m : {1, 7, 14, 22, 4097, 8192}) {
        CHECK(create(RFA_IN_U8, m, 1, h, 8, &nul) == RFA_ERR_UNSUPPORTED && nul);
        CHECK(create(RFA_IN_U8, m, 0, h, 8, &nul) == RFA_ERR_INVALID && nul);       // invalid comes first
    }
    // valid requests: the device is looked for only now (this program runs where there is none)
    for (int fmt : {RFA_IN_S8, RFA_IN_U8, RFA_IN_S16LE, RFA_IN_F32_INTERLEAVED}) {
        int st = create(fmt, 96, 25, h, 1047, &nul);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || nul);
        st = create(fmt, 4096, 4096, h, 16 * 4096, &nul);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || nul);
    }
}

static void check_null_handle() {
    CHECK(rfa_pfb_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_pfb_last_error(nullptr), "null handle") == 0);
    int32_t w[4] = {9, 9, 9, 9};
    size_t n[2] = {9, 9};
    float f[2] = {9.0f, 9.0f};
    void *s = nullptr;
    CHECK(rfa_pfb_get_plan(nullptr, w, w, w, w, 4, w) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_plan(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_taps(nullptr, f, 2, w) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_set_channels(nullptr, w, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_set_channels(nullptr, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_channels(nullptr, w, 4, w) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_max_outputs(nullptr, 1, n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_max_outputs(nullptr, 1, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_process(nullptr, f, 1, f, f, 1, n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_process(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_process_host(nullptr, f, 1, f, f, 1, n) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_process_host(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_reset(nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_stream(nullptr, &s) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w[0] == 9 && w[3] == 9 && n[0] == 9 && n[1] == 9 && f[0] == 9.0f && f[1] == 9.0f);
}

int main() {
    check_supported();
    check_create_errors();
    check_null_handle();
    if (failures) {
        std::fprintf(stderr, "pfb_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pfb_host_check ok\n");
    return 0;
}
