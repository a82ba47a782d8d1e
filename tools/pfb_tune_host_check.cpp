// Host-side check of the channelizer's fine-tuning entries that need no device:
// the table index (rfa_pfb_tuning_index, the reduction the kernel itself calls)
// against 128-bit integer arithmetic, the table (rfa_pfb_tuning_table) against
// double precision and its exact axis points, the argument errors of both, and
// the null-handle answers of rfa_pfb_set_tuning / rfa_pfb_get_tuning.  Built
// together with rfanalyzer_amd/csrc/channelizer.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
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

static const int32_t kQ[] = {1, 2, 3, 7, 96, 3840, 96000, 1000003, (1 << 20) - 1, 1 << 20};

static int32_t want_index(int32_t q, int32_t m, uint64_t n) {
    const __int128 v = (__int128)n * m;
    __int128 r = v % q;
    if (r < 0) r += q;
    return (int32_t)r;
}

static uint64_t next(uint64_t &s) {                               // xorshift64
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

static void check_index() {
    const uint64_t lim = (uint64_t)1 << 53;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    int32_t i = -7;
    for (int32_t q : kQ) {
        const uint64_t edge_n[] = {0, 1, 15, 16, (uint64_t)q - 1, (uint64_t)q, (uint64_t)q + 1, ((uint64_t)1 << 32) - 1,
                                   (uint64_t)1 << 32, ((uint64_t)1 << 32) + 1, lim - 2, lim - 1};
        const int32_t edge_m[] = {0, 1, -1, q - 1, -(q - 1), q / 2, -(q / 2)};
        for (int32_t m : edge_m) {
            if (m <= -q || m >= q) continue;
            for (uint64_t n : edge_n) {
                CHECK(rfa_pfb_tuning_index(q, m, n, &i) == RFA_OK);
                CHECK(i == want_index(q, m, n));
            }
        }
        for (int k = 0; k < 20000; k++) {
            const int shift = 11 + (int)(next(seed) % 40);
            const uint64_t n = next(seed) >> shift;                               // every magnitude below 2^53
            const int32_t m = (int32_t)(next(seed) % (uint64_t)(2 * (int64_t)q - 1)) - (q - 1);
            CHECK(rfa_pfb_tuning_index(q, m, n, &i) == RFA_OK);
            CHECK(i >= 0 && i < q && i == want_index(q, m, n));
        }
    }
    // a run of consecutive n, as the lanes of a row see them
    for (uint64_t n = ((uint64_t)1 << 32) - 40; n < ((uint64_t)1 << 32) + 40; n++) {
        CHECK(rfa_pfb_tuning_index(1 << 20, (1 << 20) - 1, n, &i) == RFA_OK && i == want_index(1 << 20, (1 << 20) - 1, n));
        CHECK(rfa_pfb_tuning_index(96000, -47999, n, &i) == RFA_OK && i == want_index(96000, -47999, n));
    }
    // argument errors leave *i alone
    i = 1234;
    CHECK(rfa_pfb_tuning_index(0, 0, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(-3, 1, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(RFA_PFB_TUNE_MAX_STEPS + 1, 1, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, 7, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, -7, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(1, 1, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, INT32_MIN, 5, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, 3, lim, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, 3, UINT64_MAX, &i) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_index(7, 3, 5, nullptr) == RFA_ERR_INVALID);
    CHECK(i == 1234);
    CHECK(rfa_pfb_tuning_index(RFA_PFB_TUNE_MAX_STEPS, RFA_PFB_TUNE_MAX_STEPS - 1, lim - 1, &i) == RFA_OK);
    CHECK(rfa_pfb_tuning_index(1, 0, lim - 1, &i) == RFA_OK && i == 0);
}

static void check_table() {
    for (int32_t q : kQ) {
        std::vector<float> c((size_t)q, 9.0f), s((size_t)q, 9.0f);   // exactly q entries: ASan sees a write past them
        CHECK(rfa_pfb_tuning_table(q, c.data(), s.data(), (size_t)q) == RFA_OK);
        double worst = 0.0;
        for (int32_t i = 0; i < q; i++) {
            const double ang = 2.0 * M_PI * (double)i / (double)q;
            worst = std::fmax(worst, std::fmax(std::fabs((double)c[(size_t)i] - std::cos(ang)),
                                               std::fabs((double)s[(size_t)i] - std::sin(ang))));
        }
        CHECK(worst <= std::ldexp(1.0, -23));
        CHECK(c[0] == 1.0f && s[0] == 0.0f);
        if (q % 4 == 0) {
            CHECK(c[(size_t)q / 4] == 0.0f && s[(size_t)q / 4] == 1.0f);
            CHECK(c[(size_t)q / 2] == -1.0f && s[(size_t)q / 2] == 0.0f);
            CHECK(c[3 * (size_t)q / 4] == 0.0f && s[3 * (size_t)q / 4] == -1.0f);
        }
        for (int32_t i = 1; i < q; i++)                               // the symmetry the octant reduction gives
            CHECK(c[(size_t)i] == c[(size_t)(q - i)] && s[(size_t)i] == -s[(size_t)(q - i)]);
        if (q > 1) {
            std::vector<float> shortc((size_t)q - 1, 9.0f), shorts((size_t)q - 1, 9.0f);
            CHECK(rfa_pfb_tuning_table(q, shortc.data(), shorts.data(), (size_t)q - 1) == RFA_ERR_SIZE);
            CHECK(shortc[0] == 9.0f && shorts[0] == 9.0f);
        }
    }
    float c = 5.0f, s = 5.0f;
    CHECK(rfa_pfb_tuning_table(0, &c, &s, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_table(-1, &c, &s, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_table(RFA_PFB_TUNE_MAX_STEPS + 1, &c, &s, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_table(1, nullptr, &s, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_table(1, &c, nullptr, 1) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_tuning_table(1, &c, &s, 0) == RFA_ERR_SIZE);
    CHECK(c == 5.0f && s == 5.0f);
    CHECK(rfa_pfb_tuning_table(1, &c, &s, 1) == RFA_OK && c == 1.0f && s == 0.0f);
}

static void check_null_handle() {
    const int32_t steps[2] = {1, -1};
    int32_t q = 9, count = 9, out[2] = {9, 9};
    CHECK(rfa_pfb_set_tuning(nullptr, 7, steps, 2) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_set_tuning(nullptr, 0, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_tuning(nullptr, &q, out, 2, &count) == RFA_ERR_INVALID);
    CHECK(rfa_pfb_get_tuning(nullptr, nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(q == 9 && count == 9 && out[0] == 9 && out[1] == 9);
}

int main() {
    check_index();
    check_table();
    check_null_handle();
    if (failures) {
        std::fprintf(stderr, "pfb_tune_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pfb_tune_host_check ok\n");
    return 0;
}
