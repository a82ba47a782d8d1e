// Host-side check of the polyphase channelizer's C-ABI entries that need no
// device: the length rule, the tile-plan query over every supported length, and
// every error path that returns before any HIP call.
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

// rfa_pfb_tile_plan over every supported M with a grid of (L, D, T) at the limits of the create
// entries: the invariants every plan has, whatever the planning rule is, and the argument errors.
static void check_tile_plan() {
    constexpr int F = RFA_PFB_PLAN_FIELDS;
    int32_t guard[F + 2];
    int32_t *w = guard + 1;
    auto fill = [&] { for (int i = 0; i < F + 2; i++) guard[i] = -77; };
    auto untouched = [&] {
        for (int i = 0; i < F + 2; i++)
            if (guard[i] != -77) return false;
        return true;
    };
    long plans = 0;
    for (int32_t m = RFA_PFB_MIN_CHANNELS; m <= RFA_PFB_MAX_CHANNELS; m++) {
        if (!smooth(m)) continue;
        for (int32_t l : {0, 1, 2, 3, 17, RFA_PFB_MAX_INTERPOLATION}) {
            const long long lm = (long long)(l ? l : 1) * m;
            const int32_t ds[] = {l ? l : 1, (l ? l : 1) + 1, (int32_t)(lm / 2) + 1, (int32_t)lm - 1, (int32_t)lm};
            const int32_t ts[] = {1, m - 1, m, 2 * m + 1, (int32_t)(RFA_PFB_MAX_PHASES * lm)};
            for (int32_t d : ds)
                for (int32_t t : ts) {
                    fill();
                    const int st = rfa_pfb_tile_plan(m, l, d, t, w);
                    if (st != RFA_OK) {                     // a (L, D) of the grid with a common factor
                        CHECK(st == RFA_ERR_INVALID && l > 1 && untouched());
                        continue;
                    }
                    plans++;
                    CHECK(guard[0] == -77 && guard[F + 1] == -77);
                    const int nt = w[RFA_PFB_PLAN_TIMES], mp = w[RFA_PFB_PLAN_PITCH];
                    CHECK(nt >= 1 && nt <= 16 && (nt & (nt - 1)) == 0 && nt * m <= 4096 && (nt == 16 || 2 * nt * m > 4096));
                    CHECK(mp >= m && mp % 2 == 1 && mp <= m + 1);
                    CHECK(w[RFA_PFB_PLAN_LDS_BYTES] == 8 * (w[RFA_PFB_PLAN_STAGE_POINTS] + 2 * nt * mp));
                    CHECK(w[RFA_PFB_PLAN_LDS_BYTES] <= 64 * 1024 + 2 * (4096 + 16) * 8);   // what the kernels are prepared for
                    CHECK(w[RFA_PFB_PLAN_STAGED_RUN] == 0 || w[RFA_PFB_PLAN_STAGED_RUN] == 1);
                    CHECK((w[RFA_PFB_PLAN_STAGE_POINTS] != 0) == (w[RFA_PFB_PLAN_STAGED_RUN] == 1));
                    CHECK(w[RFA_PFB_PLAN_STAGED_RUN] == 0 || w[RFA_PFB_PLAN_STAGE_POINTS] >= w[RFA_PFB_PLAN_RUN]);
                    CHECK(w[RFA_PFB_PLAN_STAGED_TAPS] >= 0 && w[RFA_PFB_PLAN_STAGED_TAPS] <= (l ? nt : 1));
                    CHECK(w[RFA_PFB_PLAN_STAGED_TAPS] == 0 || w[RFA_PFB_PLAN_STAGED_RUN] == 1);
                    CHECK(w[RFA_PFB_PLAN_ROWS_BY_TIME] == (l > nt && w[RFA_PFB_PLAN_STAGED_TAPS] > 0 ? 1 : 0));
                    const int ns = w[RFA_PFB_PLAN_STAGES];
                    CHECK(ns >= 1 && ns <= RFA_PFB_PLAN_MAX_STAGES);
                    long long prod = 1;
                    for (int s = 0; s < RFA_PFB_PLAN_MAX_STAGES; s++) {
                        const int r = w[RFA_PFB_PLAN_RADIX0 + s];
                        if (s < ns) {
                            CHECK(r >= 2 && r <= 5);
                            prod *= r;
                        } else {
                            CHECK(r == 0);
                        }
                    }
                    CHECK(prod == m);
                }
        }
    }
    CHECK(plans > 10000);
    // argument errors: the create entries' rules, invalid before unsupported, nothing written
    fill();
    CHECK(rfa_pfb_tile_plan(16, 0, 4, 16, nullptr) == RFA_ERR_INVALID);
    const int32_t bad[][4] = {{0, 0, 1, 16},   {-16, 0, 1, 16}, {16, 0, 0, 16},  {16, 0, -3, 16},  {16, 0, 17, 16},
                              {16, 0, 4, 0},   {16, 0, 4, -1},  {16, 0, 4, 257}, {16, -1, 4, 16},  {7, 0, 0, 8},
                              {16, 65, 66, 61}, {16, 8, 7, 61}, {16, 3, 49, 61}, {16, 6, 14, 61},  {16, 3, 7, 769},
                              {16, 3, 0, 61},  {0, 3, 7, 61},   {16, 3, 7, 0},   {7, 3, 22, 61}};
    for (const auto &a : bad) CHECK(rfa_pfb_tile_plan(a[0], a[1], a[2], a[3], w) == RFA_ERR_INVALID && untouched());
    for (int32_t m : {1, 7, 14, 22, 4097, 8192}) {
        CHECK(rfa_pfb_tile_plan(m, 0, 1, 8, w) == RFA_ERR_UNSUPPORTED && untouched());
        CHECK(rfa_pfb_tile_plan(m, 1, 1, 8, w) == RFA_ERR_UNSUPPORTED && untouched());
    }
    CHECK(rfa_pfb_tile_plan(16, 0, 16, 256, w) == RFA_OK && rfa_pfb_tile_plan(16, 3, 47, 768, w) == RFA_OK);
    CHECK(rfa_pfb_tile_plan(16, 64, 65, 61, w) == RFA_OK);
}

int main() {
    check_supported();
    check_create_errors();
    check_null_handle();
    check_tile_plan();
    if (failures) {
        std::fprintf(stderr, "pfb_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pfb_host_check ok\n");
    return 0;
}
